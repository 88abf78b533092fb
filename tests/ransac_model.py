"""TEST INFRASTRUCTURE -- a float64 NumPy restatement of the reference's polyfit(x, y, ransac=True) (utils/isp_algos.py:345-362:
sklearn's RANSACRegressor(min_samples=int(sqrt(n))) around a LinearRegression, after setup_seed(2024)), and the synthetic
Poisson-Gaussian point sets the RANSAC tests share.  No sklearn estimator runs here: only its subset draw
(sklearn.utils.random.sample_without_replacement), which the product uses too.

The point sets are functions of np.random.RandomState(seed) alone (the legacy stream is stable), so tests/golden/ransac.npz holds
results only: tools/gen_golden_ransac.py feeds the same arrays to the reference.

ADMISSIBLE winner-identity cases: the winner of sklearn's loop is decided by integer inlier counts, and a count can move by the
number of points whose residual lies within rounding of the threshold.  `fit` reports the margin (the winner's count minus the
largest count among the other trials that ran) beside the number of points with |r - thr| <= 1e-6 thr in either of the two trials;
a case is admissible when margin > borderline.  Residual errors are ~1e-10 thr here (float64 line, |y| <= ~1e2 thr), far inside
the 1e-6 band, so an admissible case has one winner whatever the summation order of an implementation.
"""
import numpy as np

BETA1, BETA2 = 3e-3, 4e-5
TRIALS, SEED = 100, 2024

# name -> (seed, n, share of contaminated points, x range, winner identity is asserted)
CASES = {
    "n300_c30": dict(seed=102, n=300, contam=0.30, lo=0.01, hi=0.70, winner=True),
    "n4096_c20": dict(seed=100, n=4096, contam=0.20, lo=0.01, hi=0.70, winner=True),
    "n5000_c20": dict(seed=102, n=5000, contam=0.20, lo=0.01, hi=0.70, winner=True),      # 5 compaction tiles, 3 scoring chunks, neither whole
    "n64_early": dict(seed=176, n=64, contam=0.05, lo=0.01, hi=0.70, winner=True),        # nearly all inliers: the dynamic rule stops after 8 trials
    "n3000_mask": dict(seed=101, n=3000, contam=0.20, lo=-0.05, hi=0.95, winner=True),    # ~20 % of x outside (1e-4, 0.8): the mask applies
    "n1500_nomask": dict(seed=100, n=1500, contam=0.20, lo=0.81, hi=1.00, winner=True, inside=9),   # 9 of 1500 qualify (< 1 %): all kept
    "n4096_clean": dict(seed=17, n=4096, contam=0.0, lo=0.01, hi=0.70, winner=False),    # near-tied counts: threshold and trial table only
}


def make_points(name):
    """(x, y) float32 of a case, before polyfit's non-saturation rule: y = (beta1 x + beta2)(1 + 0.05 z), a share of the points with
    their variance raised by a factor 1.5 .. 4 (texture inside the "flat" mask)."""
    c = CASES[name]
    rs = np.random.RandomState(c["seed"])
    n = c["n"]
    x = rs.uniform(c["lo"], c["hi"], n)
    if "inside" in c:
        x[rs.choice(n, c["inside"], replace=False)] = rs.uniform(0.1, 0.7, c["inside"])
    y = (BETA1 * np.abs(x) + BETA2) * (1.0 + 0.05 * rs.standard_normal(n))
    bad = rs.uniform(size=n) < c["contam"]
    y = np.where(bad, y * rs.uniform(1.5, 4.0, n), y)
    return x.astype(np.float32), y.astype(np.float32)


def nonsat(x, y):
    """utils/isp_algos.py:348-350."""
    keep = np.logical_and(x > 1e-4, x < 0.8)
    if len(x[keep]) > 0.01 * len(x.reshape(-1)):
        return x[keep], y[keep], True
    return x, y, False


def draw_subsets(n, m, trials=TRIALS, seed=SEED):
    from sklearn.utils.random import sample_without_replacement
    rs = np.random.RandomState(seed)
    return np.stack([sample_without_replacement(n, m, random_state=rs) for _ in range(trials)])


def mad_threshold(y):
    """sklearn's default residual_threshold on the float32 y the reference hands over: float32 all the way."""
    y = np.asarray(y, np.float32)
    return np.median(np.abs(y - np.median(y)))


def dynamic_max_trials(n_inliers, n, m, probability=0.99):
    eps = np.spacing(1)
    ratio = n_inliers / float(n)
    nom = max(eps, 1 - probability)
    denom = max(eps, 1 - ratio ** m)
    if denom == 1:
        return float("inf")
    return abs(float(np.ceil(np.log(nom) / np.log(denom))))


def r2(y, pred):
    num = ((y - pred) ** 2).sum()
    den = ((y - y.mean()) ** 2).sum()
    if den == 0:
        return 1.0 if num == 0 else 0.0
    return 1.0 - num / den


def fit(x, y, trials=TRIALS, seed=SEED):
    """dict(res, winner, n_inliers, n_trials, thr, n, m, lines [T][2], counts [T], near [T] (points within the 1e-6 band of the
    threshold, per trial), margin, borderline, masked, and the points (x, y) after the non-saturation rule)."""
    x, y, masked = nonsat(np.asarray(x, np.float32), np.asarray(y, np.float32))
    n = len(x)
    m = int(np.sqrt(n))
    thr32 = mad_threshold(y)
    thr = np.float64(thr32)
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    idx = draw_subsets(n, m, trials, seed)
    lines = np.empty((trials, 2))
    counts = np.empty(trials, np.int64)
    resid = np.empty((trials, n))
    for t in range(trials):
        A = np.stack([xd[idx[t]], np.ones(m)], axis=1)
        lines[t] = np.linalg.lstsq(A, yd[idx[t]], rcond=None)[0]
        resid[t] = np.abs(yd - (lines[t, 0] * xd + lines[t, 1]))
        counts[t] = int((resid[t] <= thr).sum())
    best, n_best, score_best = -1, 1, -np.inf
    max_trials, run = trials, 0
    while run < max_trials:
        t = run
        run += 1
        if counts[t] < n_best:
            continue
        inl = resid[t] <= thr
        score = r2(yd[inl], lines[t, 0] * xd[inl] + lines[t, 1])
        if counts[t] == n_best and score < score_best:
            continue
        best, n_best, score_best = t, int(counts[t]), score
        max_trials = min(max_trials, dynamic_max_trials(n_best, n, m))
    assert best >= 0
    inl = resid[best] <= thr
    A = np.stack([xd[inl], np.ones(int(inl.sum()))], axis=1)
    res = np.linalg.lstsq(A, yd[inl], rcond=None)[0]
    others = [t for t in range(run) if t != best]
    second = max(others, key=lambda t: counts[t]) if others else best
    band = 1e-6 * thr
    near = lambda t: int((np.abs(resid[t] - thr) <= band).sum())
    return dict(res=res, winner=best, n_inliers=n_best, n_trials=run, thr=thr32, n=n, m=m, lines=lines, counts=counts, idx=idx,
                margin=(n_best - int(counts[second])) if others else n_best, borderline=near(best) + (near(second) if others else 0),
                borderline_all=int((np.abs(resid[:run] - thr) <= band).sum()), near=(np.abs(resid - thr) <= band).sum(axis=1), masked=masked,
                x=x, y=y)
