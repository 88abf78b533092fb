"""A plain Python / NumPy model of the device frame chain's parameter block (csrc/frame_params.h), written from the reference's
expressions -- utils/isp_algos.py:345-365 (polyfit) and :98-108 (get_bias' knot grid), YOND_SIDD.py:79-84 (no flat area),
:341-356 (round 1), :438-454 (round 2), :263-268 / :284-285 (lower, upper, nsr, t) -- as the oracle restates them (polyfit, VST,
bias_knots, IterDenoise).  tests/test_chain_model.py holds the model to the oracle on the CPU; tests/test_hip_chain_params.py
holds the kernels to the model."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53                                   # unit roundoff of float64
NO_FLAT_AREA, LUT_CAPACITY, ROUND_ABORTED, BAD_ESTIMATE = 1, 2, 4, 8
BIAS_DEV_SMEM_DOUBLES = 6144                     # LDS doubles of yond_bias_lut_dev_f64 / yond_frame_chain_f64 (48 KB)


def moments_of(points):
    """The estimator's ten sums from explicit (mean, var) points: {n, Sm, Sv, Smm, Smv} over all points and over the non-saturated
    ones (1e-4 < mean < 0.8, utils/isp_algos.py:348), each sum by math.fsum (correctly rounded).  Returns (m_all, m_ns)."""
    def sums(pts):
        return np.array([float(len(pts)), math.fsum(m for m, _ in pts), math.fsum(v for _, v in pts),
                         math.fsum(m * m for m, _ in pts), math.fsum(m * v for m, v in pts)], np.float64)
    pts = [(float(m), float(v)) for m, v in points]
    return sums(pts), sums([(m, v) for m, v in pts if 1e-4 < m < 0.8])


def fit(m_all, m_ns):
    """utils/isp_algos.py:345-365 on the moment sums: the non-saturated set when it holds MORE than 1 % of the points (:349, strict,
    in float64), then the least-squares line v = b1 m + b2.  Returns a dict:
      b1, b2   the EXACT solution of the 2x2 normal equations on the given float64 sums (fractions.Fraction; float NaN when a sum
               is not finite),
      e1, e2   a forward error bound for a float64 evaluation of  b1 = (n Smv - Sm Sv) / det,  b2 = (Smm Sv - Sm Smv) / det,
               det = n Smm - Sm^2:  4u (|n Smv| + |Sm Sv|) / |det|  for the numerator plus  4u |b| (n Smm + Sm^2) / |det|  for the
               determinant, u = 2^-53.  The factor 4 COUNTS roundings (two products, one subtraction, one division, each at most
               u relative to the larger terms); it is derived, not measured,
      used     'ns' or 'all',  branch  'fit', 'rank' or 'empty'.
    Rank-deficient designs (n < 2, or det <= 1e-12 max(n Smm, 1e-300), evaluated in Python floats in the kernel's operation
    order): scipy.linalg.lstsq (:364) returns the minimum-norm solution vbar (mbar, 1) / (mbar^2 + 1); the bound there counts
    eight roundings (mbar, vbar, their product, the square, the sum, the quotient).  n <= 0: (0, 0)."""
    m_all = [float(v) for v in m_all]
    m_ns = [float(v) for v in m_ns]
    used = 'ns' if m_ns[0] > 0.01 * m_all[0] else 'all'
    n, sx, sy, sxx, sxy = m_ns if used == 'ns' else m_all
    nsxx = n * sxx
    det = nsxx - sx * sx
    lim = nsxx if nsxx > 1e-300 else 1e-300
    out = dict(used=used, det=det, lim=lim)
    if n < 2.0 or det <= 1e-12 * lim:
        if n <= 0.0:
            return dict(out, branch='empty', b1=Fraction(0), b2=Fraction(0), e1=0.0, e2=0.0)
        if not all(math.isfinite(v) for v in (n, sx, sy)):
            return dict(out, branch='rank', b1=math.nan, b2=math.nan, e1=math.nan, e2=math.nan)
        mbar, vbar = Fraction(sx) / Fraction(n), Fraction(sy) / Fraction(n)
        b1, b2 = vbar * mbar / (mbar * mbar + 1), vbar / (mbar * mbar + 1)
        g8 = 8 * U / (1 - 8 * U)
        return dict(out, branch='rank', b1=b1, b2=b2, e1=g8 * abs(float(b1)), e2=g8 * abs(float(b2)))
    if not all(math.isfinite(v) for v in (n, sx, sy, sxx, sxy)):
        return dict(out, branch='fit', b1=math.nan, b2=math.nan, e1=math.nan, e2=math.nan)
    N, SX, SY, SXX, SXY = (Fraction(v) for v in (n, sx, sy, sxx, sxy))
    D = N * SXX - SX * SX
    b1, b2 = (N * SXY - SX * SY) / D, (SXX * SY - SX * SXY) / D
    ad = abs(float(D))
    dpart = 4 * U * (n * sxx + sx * sx) / ad
    e1 = 4 * U * (abs(n * sxy) + abs(sx * sy)) / ad + dpart * abs(float(b1))
    e2 = 4 * U * (abs(sxx * sy) + abs(sx * sxy)) / ad + dpart * abs(float(b2))
    return dict(out, branch='fit', b1=b1, b2=b2, e1=e1, e2=e2)


def _vst0(x, sigma, gain):
    """utils/isp_algos.py:5-14 with mu = 0 on float64 scalars."""
    fz = gain * x + (3 / 8) * gain ** 2 + sigma ** 2
    fz = np.maximum(fz, 0)
    return 2 / gain * np.sqrt(fz)


def params(b1, b2, mode, scale_est, scale, tfac, n_all=None):
    """(beta1, beta2) -> the frame's constants.  mode 0 is round 1 (YOND_SIDD.py:356: K = b1 scale, sigma = sqrt(max(b2, 0)) scale),
    mode 1 round 2 (:438-447: b2 < 0 -> b1^2, sigma = sqrt(b2) scale, b1 < 0 ends the image: ROUND_ABORTED).  lower = VST(0),
    upper = VST(scale), nsr = 1 / (upper - lower) (:264-268), t = float32(nsr * tfac) (:284-285).
    Returns dict(b2 (as stored), gain, sigma, lo, hi, nsr: float64; t: float32; flags).  BAD_ESTIMATE: not (gain > 0) or
    not (sigma >= 0), NaN included; NO_FLAT_AREA (n_all given): not (n_all > 0), YOND_SIDD.py:79-84."""
    b1, b2 = np.float64(b1), np.float64(b2)
    scale_est, scale, tfac = np.float64(scale_est), np.float64(scale), np.float64(tfac)
    flags = 0
    with np.errstate(all='ignore'):
        if mode == 0:
            gain, sigma = b1 * scale_est, np.sqrt(np.maximum(b2, 0)) * scale_est
            if np.isnan(b2):                         # (Python's max(b2, 0) of the reference keeps a NaN b2)
                sigma = np.float64(np.nan)
        elif mode == 1:
            if b2 < 0:
                b2 = b1 ** 2
            gain, sigma = b1 * scale_est, np.sqrt(b2) * scale_est
            if b1 < 0:
                flags |= ROUND_ABORTED
        else:
            raise ValueError(mode)
        if not (gain > 0) or not (sigma >= 0):
            flags |= BAD_ESTIMATE
        if n_all is not None and not (n_all > 0):
            flags |= NO_FLAT_AREA
        lo, hi = _vst0(np.float64(0.0), sigma, gain), _vst0(scale, sigma, gain)
        nsr = 1 / (hi - lo)
        t = np.float32(nsr * tfac)
    return dict(b2=np.float64(b2), gain=np.float64(gain), sigma=np.float64(sigma), lo=np.float64(lo), hi=np.float64(hi),
                nsr=np.float64(nsr), t=t, flags=flags)


def knot_shape(frame_max_f32, scale, lut_cap):
    """The shape of get_bias' knot grid (utils/isp_algos.py:101-108) for ub = float32(ceil(float32(max) * float32(scale))) + 1:
    ((n1, n2, n3, nk), flags).  NumPy 2 keeps `ub` in float32 through (ub - lb) / 0.1, ub - 50 and ub - 500.  LUT_CAPACITY: more
    knots than the buffers hold, or not (ub >= 0) (a negative or NaN maximum); the shape is then all zeros."""
    with np.errstate(all='ignore'):
        ub = np.float32(np.ceil(np.float32(frame_max_f32) * np.float32(scale))) + np.float32(1)
    if not (ub >= 0):
        return (0, 0, 0, 0), LUT_CAPACITY
    lb = 0
    if ub < 50:
        n1, n2, n3 = int((ub - lb) / 0.1) + 2, 0, 0
    elif ub < 500:
        n1, n2, n3 = int((50 - lb) / 0.1) + 1, int(ub - 50) + 2, 0
    else:
        n1, n2, n3 = int((50 - lb) / 0.1) + 1, 451, int(ub - 500) // 10 + 2
    nk = n1 + n2 + n3
    if nk > lut_cap:
        return (0, 0, 0, 0), LUT_CAPACITY
    return (n1, n2, n3, nk), 0


def lds_doubles(K, sigma):
    """LDS doubles the integration of a bias LUT needs, with pho, th and rmax as yond_bias_lut_f64 derives them
    (utils/isp_algos.py:112, :115, :123 at the largest integrated knot): the Gaussian table 2 pho rmax + 1, the Poisson masses
    rmax + 1, one spare."""
    pho = max(int(math.sqrt(K)), 1)
    th = 50.0 * K if K < 1.0 else 50.0 * math.sqrt(K)
    rmax = int(th * (1.0 / K) * 2.0 + sigma * 2.0 + th + 10.0) + 1
    return 2 * pho * rmax + 1 + rmax + 2


def float2key(x):
    """The kernels' order-preserving 32-bit key of a float32 (inverse of pipeline._key2float): negative floats complemented,
    the others with the top bit set."""
    b = int(np.array([x], np.float32).view(np.uint32)[0])
    return (~b & 0xFFFFFFFF) if (b & 0x80000000) else (b | 0x80000000)


def ulps64(a, b):
    """Distance of two float64 in units in the last place (0 for equal values and for two NaNs, inf where only one is NaN or the
    signs of two infinities differ)."""
    a, b = np.float64(a), np.float64(b)
    if np.isnan(a) or np.isnan(b):
        return 0.0 if (np.isnan(a) and np.isnan(b)) else math.inf
    if a == b:
        return 0.0
    if np.isinf(a) or np.isinf(b):
        return math.inf

    def order(v):
        i = int(np.array([v], np.float64).view(np.int64)[0])
        return i if i >= 0 else -(i & 0x7FFFFFFFFFFFFFFF)
    return float(abs(order(a) - order(b)))


def ulps32(a, b):
    a, b = np.float32(a), np.float32(b)
    if np.isnan(a) or np.isnan(b):
        return 0.0 if (np.isnan(a) and np.isnan(b)) else math.inf
    if a == b:
        return 0.0
    if np.isinf(a) or np.isinf(b):
        return math.inf

    def order(v):
        i = int(np.array([v], np.float32).view(np.int32)[0])
        return i if i >= 0 else -(i & 0x7FFFFFFF)
    return float(abs(order(a) - order(b)))
