"""TEST INFRASTRUCTURE ONLY -- the float64 model of the illuminance correction (include/yond_hip.h M2; the reference's
data_process/__init__.py:158-171 IlluminanceCorrect.correct), its layouts and modes, its single-defect variants, and the seeded cases
of tests/golden/illum.npz (tools/gen_golden_illum.py runs the reference's class on them).

    p = clamp(pred, 0, 1); over the elements with source != 1:  num = sum p * source, den = sum p * p, count
    gain = float32(num / den);  out = float32(gain * p)  [then min(out, 1) with clip]

Every product of two float32 values is exact in float64 and math.fsum adds them without error: num and den are the correctly rounded
sums, the gain is rounded to float32 once.
"""
import math

import numpy as np

FLAT, BAYER, PACKED4 = 'flat', 'bayer', 'packed4'
DEFECTS = ('no_clamp', 'mask_ignored', 'mask_on_pred', 'mask_lt', 'den_ps', 'gain_on_unclamped', 'groups_transposed')


def clamp01(x):
    """torch.clamp(x, 0, 1) in float32: a NaN stays a NaN."""
    x = np.asarray(x, np.float32)
    return np.where(x < 0, np.float32(0), np.where(x > 1, np.float32(1), x)).astype(np.float32)


def groups(shape, layout, width=None):
    """int array of `shape` (flat order): the group 0..3 of every element."""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.int64)
    if layout == FLAT:
        g = np.zeros(n, np.int64)
    elif layout == PACKED4:
        g = i & 3
    elif layout == BAYER:
        w = int(width if width is not None else shape[-1])
        g = ((i // w) & 1) * 2 + ((i % w) & 1)
    else:
        raise ValueError(layout)
    return g.reshape(shape)


def _fsum(a):
    a = np.asarray(a, np.float64).reshape(-1)
    if np.isnan(a).any():
        return float('nan')
    return math.fsum(a.tolist())


def sums(pred, source, layout=FLAT, width=None, defect=None):
    """float64 [5][3]: {num, den, count} of the four groups and, in row 4, of the frame (fsum over everything included, not the sum of
    the four rounded group sums)."""
    pred, source = np.asarray(pred, np.float32), np.asarray(source, np.float32)
    p = pred if defect == 'no_clamp' else clamp01(pred)
    if defect == 'mask_ignored':
        mask = np.ones(source.shape, bool)
    elif defect == 'mask_on_pred':
        mask = p != 1
    elif defect == 'mask_lt':
        mask = source < 1
    else:
        mask = source != 1
    g = groups(pred.shape, layout, width)
    if defect == 'groups_transposed':
        g = np.array([0, 2, 1, 3])[g]
    pd, sd = p.astype(np.float64), source.astype(np.float64)
    num_t, den_t = pd * sd, (pd * sd if defect == 'den_ps' else pd * pd)
    out = np.zeros((5, 3), np.float64)
    for k in range(5):
        m = mask if k == 4 else (mask & (g == k))
        out[k] = (_fsum(num_t[m]), _fsum(den_t[m]), float(m.sum()))
    return out


def gain_of(row):
    """float32(num / den) of one row of sums, IEEE: 0 / 0 is NaN, x / 0 an infinity."""
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.float32(np.float64(row[0]) / np.float64(row[1]))


def apply(pred, s, mode='frame', clip=False, layout=FLAT, width=None, defect=None):
    """float32 out = gain * clamp(pred, 0, 1) with the gains of s (a [5][3] sums array)."""
    pred = np.asarray(pred, np.float32)
    p = pred if defect in ('no_clamp', 'gain_on_unclamped') else clamp01(pred)
    if mode == 'frame':
        gain = gain_of(s[4])
    else:
        g = groups(pred.shape, layout, width)
        if defect == 'groups_transposed':
            g = np.array([0, 2, 1, 3])[g]
        gain = np.array([gain_of(s[k]) for k in range(4)], np.float32)[g]
    with np.errstate(invalid='ignore', over='ignore'):
        out = (gain * p).astype(np.float32)
    if clip:
        out = np.where(out > 1, np.float32(1), out).astype(np.float32)
    return out


def correct(pred, source, mode='frame', clip=False, layout=FLAT, width=None, defect=None):
    """(out, sums) of one item."""
    s = sums(pred, source, layout, width, defect)
    return apply(pred, s, mode, clip, layout, width, defect), s


def forward(predict, source, defect=None):
    """The reference's forward for [N][C][H][W]: per item, FLAT, a batch-1 source shared."""
    predict, source = np.asarray(predict, np.float32), np.asarray(source, np.float32)
    return np.stack([correct(predict[i], source[i if source.shape[0] != 1 else 0], defect=defect)[0] for i in range(predict.shape[0])])


def out_bound(n):
    """Relative bound on |reference out - model out| for n included elements: 2 (n - 1) * 2^-24 + 3 * 2^-24.  The reference forms num
    and den as float32 dots of non-negative terms.  A term is rounded once as a product and once per addition it passes through, at
    most n - 1 of them in ANY order of summation, and with no cancellation the relative error of the sum is at most that of its worst
    term: n * 2^-24 per dot (first order).  The quotient of the two is within 2 n * 2^-24, its float32 division adds 2^-24:
    the reference's gain is within (2 (n - 1) + 3) * 2^-24 of the exact one, whatever order its BLAS adds in.  (The model's one
    rounding of the gain and the final float32 multiply on either side are three more roundings of 2^-24 that this bound does not
    count; it is the worst case of a sum whose typical error grows like sqrt(n), and the measured distances, which the fixture
    records, are 1e-7 to 3e-7.)"""
    return (2.0 * (n - 1) + 3.0) * 2.0 ** -24


# ---- the fixture's seeded cases -------------------------------------------------------------------------------------------------
CASES = {                    # name -> (predict shape, source batch, seed)
    'c1_2x2': ((1, 4, 2, 2), 1, 11),
    'c2_6x10': ((1, 4, 6, 10), 1, 12),
    'c3_62x130': ((1, 4, 62, 130), 1, 13),
    'c4_batch3': ((3, 4, 8, 8), 3, 14),
    'c5_batch3_src1': ((3, 4, 8, 8), 1, 15),
}


def make_case(name):
    """(predict, source) float32 of a case, a function of its seed alone.  The targets are a scene in (0, 1) with 7.5 % of them exactly
    1.0 (2 x 2 case: one), some at nextafter(1, 0) and some above 1 (1.5 .. 2.5); the prediction is target / 1.25 + a black-level
    offset + noise (true gain 1.25: away from 1), carries no information where the target is saturated (0.2 .. 0.6 there: the scene
    was brighter than the target can say), and 3.5 % of it lies far outside [0, 1] (3.0 and -2.0)."""
    shape, nsrc, seed = CASES[name]
    rng = np.random.RandomState(seed)
    sshape = (nsrc,) + tuple(shape[1:])
    source = rng.uniform(0.02, 0.95, sshape).astype(np.float32)
    n = source.size
    u = rng.permutation(n)
    flat = source.reshape(-1)
    n_sat = max(1, int(round(0.075 * n)))
    n_below, n_above = max(1, n // 50), max(1, n // 50)
    flat[u[:n_sat]] = np.float32(1.0)
    flat[u[n_sat:n_sat + n_below]] = np.nextafter(np.float32(1), np.float32(0))
    flat[u[n_sat + n_below:n_sat + n_below + n_above]] = rng.uniform(1.5, 2.5, n_above).astype(np.float32)
    src_b = np.broadcast_to(source, shape)
    predict = (src_b / np.float32(1.25) + np.float32(0.013) + rng.normal(0.0, 0.02, shape)).astype(np.float32)
    predict = np.where(src_b == 1, rng.uniform(0.2, 0.6, shape), predict).astype(np.float32)
    pf = predict.reshape(-1)
    v = rng.permutation(pf.size)
    n_out = max(2, int(round(0.035 * pf.size)))
    pf[v[:n_out // 2]] = np.float32(3.0)
    pf[v[n_out // 2:n_out]] = np.float32(-2.0)
    return predict, np.ascontiguousarray(source)


def exercises(name, defect):
    """True where a case's data can tell `defect` from the model at all (the generator and the CPU test assert it does)."""
    return defect != 'groups_transposed'                             # FLAT has one group: the transposition is checked on BAYER / PACKED4


def rel_dist(got, ref):
    """max over the elements of |got - ref| / |ref| (0 where both are 0, inf where only ref is; NaNs must coincide)."""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaNs at different places"
    ok = ~np.isnan(ref)
    got, ref = got[ok], ref[ok]
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(ref != 0, np.abs(got - ref) / np.abs(ref), np.where(got != 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def assert_within(got, ref, bound, what):
    d = rel_dist(got, ref)
    assert d <= bound, f"{what}: relative distance {d:.3e} above the bound {bound:.3e}"
    return d


def assert_outside(ref_out, defect_out, predict, source, what):
    """A defect variant must be told from the reference on EVERY item by more than the item's bound."""
    for i in range(predict.shape[0]):
        n_incl = int((source[i if source.shape[0] != 1 else 0] != 1).sum())
        d = rel_dist(defect_out[i], ref_out[i])
        assert d > out_bound(n_incl), f"{what}[{i}]: the defect is only {d:.3e} away, inside the bound {out_bound(n_incl):.3e}"
