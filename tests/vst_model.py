"""Plain float64 references of K1 (yond_pack_vst_norm*), K4 (yond_denorm_ivst_unpack*) and N1 (yond_block_metrics_f32), the
per-element bound the header promises for K1 / K4, and the case lists of the edge tests.  NumPy only, independent of the library.

K1 (include/yond_hip.h): "the result differs from the staged float64 evaluation by at most one float32 ulp, and only where that
evaluation lies within 1e-12 of a rounding boundary".  The staged evaluation (YOND_SIDD.py:251-269, utils/isp_algos.py:5-14, 128):

    x32 = float32(x) * float32(scale)                                   one float32 product
    vst = 2/K * sqrt(max(K x32 + 3/8 K^2 + sigma^2, 0))                  float64
    v   = vst - bias(max(x32, 0))                                        float64; the LUT as interp1d evaluates it
    u   = clamp(reflect_pad((v - lo) / (hi - lo)), 0, 1)                 float64, then ONE rounding to float32

    band = 1e-12 * (|vst| + |bias| + |lo|) / (hi - lo)

is the header's "1e-12 relative" of each of the three shortcuts (the root, the LUT as a + b x, the reciprocal span) carried to u.
One more term, which csrc/lut_table.h admits: a query within 1e-3 of a step of a knot may be evaluated on the neighbouring
interval of the (continuous) LUT, which differs from the right one by the change of slope times the distance to the knot:

    band += |slope_next - slope_prev| * |x - knot| / (hi - lo)            for |x - knot| <= 1e-3 * step, from the knots alone.

Where the unclamped value lies beyond [0, 1] by more than its band the clamp leaves one answer, 0 or 1 exactly: band = 0 there.

K4 (utils/isp_algos.py:17-33 restated in float64): z = clamp(y, 0, 1) * (hi - lo) + lo, the algebraic or the closed-form inverse,
max(., 0), * gain / scale, optional clip to [0, 1], ONE rounding.  band = 8 * 2^-53 * (sum of the |terms| of the form) * gain / scale:
eight float64 roundings of the largest term (the kernel forms z^-2 and z^-3 by multiplication where NumPy calls pow).

ulp_check(got32, v64, band) asserts |got32 - v64| <= ulp32(v64) / 2 + band for EVERY element: outside the band around a rounding
midpoint only the correctly rounded float32 passes, inside it either neighbour does.

N1: SSIM as YOND_SIDD.py:679-697 computes it (x255 as a float32 product, 11 x 11 Gaussian window of sigma 1.5, 'valid' part, C1 / C2),
written as the direct 121-tap float64 sum with the 2-D window outer(g, g) -- without the separable shortcut of csrc/metrics.hip.
"""
import numpy as np

SCALE = 959.0
KSIG = ((0.05, 0.3), (0.72, 1.8), (4.37, 6.27), (22.65, 37.09), (120.0, 0.0), (1.0, 400.0))
K1_DEFECTS = ('sqrt_f32', 'scale_f64', 'searchsorted_right', 'interval_off_by_one', 'symmetric', 'no_fz_clamp', 'lut_at_x')
K4_DEFECTS = ('no_z_guard',)
N1_DEFECTS = ('mask_le', 'x255_f64', 'se_42')
SHARE_MAX = 0.01                    # two-answer share of a well-conditioned case
COND_MAX = 10.0                     # (|lo| + |hi|) / (hi - lo) of a well-conditioned case


# ---------------------------------------------------------------------------------------------------------------------------
# the bound
# ---------------------------------------------------------------------------------------------------------------------------
def ulp32(v):
    """Spacing of float32 at |v| (float64 array): 2^(e - 23) for 2^e <= |v| < 2^(e+1), 2^-149 in the subnormal range and at 0."""
    a = np.abs(np.asarray(v, np.float64))
    _, e = np.frexp(a)
    return np.ldexp(1.0, np.where(a == 0, -149, np.maximum(e - 24, -149)))


def _round32(v):
    with np.errstate(over='ignore', under='ignore'):
        return np.asarray(v, np.float64).astype(np.float32)


def ulp_ratio(got32, v64, band):
    """|got - v64| / (ulp32(v64) / 2 + band) per element; a NaN on either side counts as infinitely far."""
    got, v = np.asarray(got32).astype(np.float64), np.asarray(v64, np.float64)
    with np.errstate(invalid='ignore'):
        r = np.abs(got - v) / (ulp32(v) / 2 + np.asarray(band, np.float64))
    return np.where(np.isnan(r), np.inf, r)


def two_answers(v64, band):
    """Elements for which both float32 neighbours of v64 satisfy the bound (v64 within `band` of a rounding midpoint)."""
    v = np.asarray(v64, np.float64)
    near = _round32(v)
    up = np.nextafter(near, np.float32(np.inf)).astype(np.float64)
    dn = np.nextafter(near, np.float32(-np.inf)).astype(np.float64)
    far = np.where(v >= near.astype(np.float64), up, dn)          # the neighbour on v64's side of the nearest float32
    lim = ulp32(v) / 2 + np.asarray(band, np.float64)
    return np.abs(far - v) <= lim


def ulp_stats(got32, v64, band):
    """(worst ratio, two-answer share, number of two-answer elements that took the farther neighbour)."""
    r = ulp_ratio(got32, v64, band)
    two = two_answers(v64, band)
    farther = two & (np.asarray(got32) != _round32(v64))
    return float(r.max()), float(two.mean()), int(farther.sum())


def ulp_check(got32, v64, band, name=""):
    """Asserts the bound for every element; returns the share of elements for which two answers are admissible."""
    got32 = np.asarray(got32)
    assert got32.dtype == np.float32 and got32.shape == np.shape(v64), (name, got32.dtype, got32.shape, np.shape(v64))
    r = ulp_ratio(got32, v64, band)
    bad = r > 1.0
    if bad.any():
        i = np.unravel_index(int(np.argmax(r)), r.shape)
        raise AssertionError(f"{name}: {int(bad.sum())} of {r.size} elements beyond ulp/2 + band; worst at {i}: got {got32[i]!r}, "
                             f"float64 {np.asarray(v64)[i]!r}, band {np.broadcast_to(band, r.shape)[i]:.3e}, ratio {r[i]:.4g}")
    return float(two_answers(v64, band).mean())


def well_conditioned(lo, hi):
    return (abs(lo) + abs(hi)) / (hi - lo) <= COND_MAX


# ---------------------------------------------------------------------------------------------------------------------------
# K1
# ---------------------------------------------------------------------------------------------------------------------------
def vst64(x, K, sigma):
    """utils/isp_algos.py:5-14 (mu = 0) in float64, term by term in the reference's order."""
    K, sigma = np.float64(K), np.float64(sigma)
    fz = K * np.asarray(x, np.float64) + (3 / 8) * K ** 2 + sigma ** 2
    return 2 / K * np.sqrt(np.maximum(fz, 0))


def pack(bayer):
    """utils/isp_ops.py:57-60: [H][W] -> [H/2][W/2][4] (R, G1, G2, B positions of the 2 x 2 quad)."""
    b = np.asarray(bayer)
    return np.stack((b[0::2, 0::2], b[0::2, 1::2], b[1::2, 0::2], b[1::2, 1::2]), axis=-1)


def unpack(rggb):
    h, w, _ = rggb.shape
    out = np.empty((2 * h, 2 * w), rggb.dtype)
    out[0::2, 0::2], out[0::2, 1::2], out[1::2, 0::2], out[1::2, 1::2] = (rggb[..., c] for c in range(4))
    return out


def _slopes(lx, ly32):
    """Per interval i (ending at knot i >= 1): float32 difference of the float32 ordinates over the float64 knot distance, as
    interp1d forms it (scipy _call_linear); the zero-width interval between the copies of a repeated knot has none (never selected)."""
    dy = (ly32[1:] - ly32[:-1]).astype(np.float64) if ly32.dtype == np.float32 else ly32[1:] - ly32[:-1]
    dx = lx[1:] - lx[:-1]
    with np.errstate(divide='ignore', invalid='ignore'):
        s = np.where(dx > 0, dy / dx, np.nan)
    return np.concatenate(([np.nan], s))


def lut1d(lx, ly, xq, defect=None):
    """interp1d(lx, ly)(xq), kind 'linear': hi = clip(searchsorted(lx, xq, 'left'), 1, n - 1), slope * (xq - x_lo) + y_lo.  Equal to
    np.interp inside the knots but for the ordinates' float32 difference.  Raises beyond the knots (bounds_error=True)."""
    lx, ly, xq = np.asarray(lx, np.float64), np.asarray(ly), np.asarray(xq, np.float64)
    if defect != 'lut_at_x' and xq.size and (xq.min() < lx[0] or xq.max() > lx[-1]):
        raise ValueError("A value in x_new is outside the interpolation range.")
    side = 'right' if defect == 'searchsorted_right' else 'left'
    hi = np.searchsorted(lx, xq, side)
    if defect == 'interval_off_by_one':
        hi = hi + 1
    hi = hi.clip(1, len(lx) - 1)
    if defect == 'interval_off_by_one':
        hi = np.where(lx[hi] == lx[hi - 1], hi - 1, hi)           # (not the zero-width interval: that would be a second defect)
    lo = hi - 1
    slope = _slopes(lx, ly)[hi]
    if defect == 'searchsorted_right':
        # 'right' steps over BOTH copies of a repeated knot only from above; a query equal to the last knot would index past the end
        slope = np.where(np.isnan(slope), 0.0, slope)
    return slope * (xq - lx[lo]) + ly[lo].astype(np.float64)


def knot_band(lx, ly, xq):
    """|slope_next - slope_prev| * |x - knot| for a query within 1e-3 of a step of an interior knot (csrc/lut_table.h: such a query may
    be evaluated on the neighbouring interval), 0 elsewhere.  From the knots alone."""
    lx, xq = np.asarray(lx, np.float64), np.asarray(xq, np.float64)
    s = _slopes(lx, np.asarray(ly))
    n = len(lx)
    out = np.zeros(xq.shape)
    hi = np.searchsorted(lx, xq, 'left').clip(1, n - 1)
    for k in (hi - 1, hi):                                        # the two knots of the query's interval
        # the non-empty intervals on either side of knot k (a repeated knot: skip the zero-width one)
        p = np.where((k >= 1) & (lx[k] == lx[np.maximum(k - 1, 0)]), k - 1, k)             # interval ending at the first copy
        q = np.where((k + 1 <= n - 1) & (lx[np.minimum(k + 1, n - 1)] == lx[k]), k + 2, k + 1)
        ok = (p >= 1) & (q <= n - 1)
        p, q = p.clip(1, n - 1), q.clip(1, n - 1)
        step = np.minimum(lx[p] - lx[p - 1], lx[q] - lx[q - 1])
        d = np.abs(xq - lx[k])
        hit = ok & (d <= 1e-3 * step)
        with np.errstate(invalid='ignore'):
            out = np.maximum(out, np.where(hit, np.abs(s[q] - s[p]) * d, 0.0))
    return out


def close_form_bias64(x, sigma, K):
    """utils/isp_algos.py:84-96."""
    y, sg = x / K, sigma / K
    yh = y + 3 / 8 + sg ** 2
    m1 = (y + sg ** 2) / yh ** 2
    m2 = y / yh ** 3
    m3 = (y + 3 * (y + sg ** 2) ** 2) / yh ** 4
    return 2 * yh ** 0.5 * (-1 / 8 * m1 + 1 / 16 * m2 - 5 / 128 * m3)


def lut2d(lx, ly, xq, K, sigma):
    """BiasLUT.get_lut (utils/isp_algos.py:179-194, 221-230) on the merged row ly over the knots lx (in DN): the fractional knot position
    of pos_interp, the two-ordinate merge of data_merge, the last ordinate up to one more interval beyond the last knot, and from
    there get_bias_points' closed form, rounded to the queries' float32 (:143 zeros_like(lams))."""
    lx, ly, xq = np.asarray(lx, np.float64), np.asarray(ly, np.float64), np.asarray(xq, np.float64)
    n = len(lx)
    data = np.concatenate(([-np.inf], lx))
    idx = np.searchsorted(data, xq).clip(0, n)
    with np.errstate(invalid='ignore'):
        pos = idx - (data[idx] - xq) / (data[idx] - data[idx - 1]) - 1
    beyond = pos >= n
    pc = pos.clip(0, n - 1)
    l, r = np.int32(np.floor(pc)), np.int32(np.ceil(pc))
    wr = pc - l
    bias = ly[l] * (1 - wr) + ly[r] * wr
    if beyond.any():
        bias[beyond] = close_form_bias64(xq[beyond], np.float64(sigma), np.float64(K)).astype(np.float32)
    return bias


def k1_ref(bayer, pads, mode, scale, K, sigma, lo, hi, lut_x=None, lut_y=None, biaslut=False, defect=None):
    """The staged float64 evaluation of K1 before its one rounding, and the band.  bayer [H][W] float32, pads (l, r, t, b);
    lut_x / lut_y: the knots the kernel is given (None: no bias correction).  Returns (u64, band), both [Hp][Wp][4]."""
    pl, pr, pt, pb = pads
    x = pack(np.asarray(bayer, np.float32))
    padmode = 'symmetric' if defect == 'symmetric' else 'reflect'
    pad = lambda a: np.pad(a, ((pt, pb), (pl, pr), (0, 0)), mode=padmode)
    if mode == 0:
        with np.errstate(invalid='ignore'):
            u = np.clip(pad(x.astype(np.float64)), 0, 1)
        return u, np.zeros(u.shape)
    K, sigma, lo, hi = np.float64(K), np.float64(sigma), np.float64(lo), np.float64(hi)
    with np.errstate(over='ignore', invalid='ignore'):
        if defect == 'scale_f64':
            xd = x.astype(np.float64) * np.float64(scale)
        else:
            xd = (x * np.float32(scale)).astype(np.float64)       # float32 * python float -> float32
        fz = K * xd + (3 / 8) * K ** 2 + sigma ** 2
        if defect != 'no_fz_clamp':
            fz = np.maximum(fz, 0)
        if defect == 'sqrt_f32':
            vst = 2 / K * np.sqrt(fz.astype(np.float32)).astype(np.float64)
        else:
            vst = 2 / K * np.sqrt(fz)
    bias = np.zeros(xd.shape)
    extra = np.zeros(xd.shape)
    if lut_x is not None:
        xq = xd if defect == 'lut_at_x' else np.maximum(xd, 0)
        if biaslut:
            bias = lut2d(lut_x, lut_y, xq, K, sigma)
        else:
            bias = lut1d(lut_x, lut_y, xq, defect)
            extra = knot_band(lut_x, lut_y, xq)
    span = hi - lo
    raw = pad((vst - bias - lo) / span)
    band = pad((1e-12 * (np.abs(vst) + np.abs(bias) + abs(lo)) + extra) / span)
    with np.errstate(invalid='ignore'):
        band = np.where((raw < -band) | (raw > 1 + band), 0.0, band)
        u = np.clip(raw, 0, 1)
    return u, band


# ---------------------------------------------------------------------------------------------------------------------------
# K4
# ---------------------------------------------------------------------------------------------------------------------------
def k4_ref(net_out, pad_t, pad_l, h, w, mode, scale, K, sigma, lo, hi, clip01, defect=None):
    """utils/isp_algos.py:17-33 and YOND_SIDD.py:286-299 in float64 before the one rounding.  net_out [Hp][Wp][4] float32.
    Returns (r64, band), both [2h][2w]."""
    y = np.asarray(net_out, np.float32)[pad_t:pad_t + h, pad_l:pad_l + w]
    with np.errstate(invalid='ignore'):
        yc = np.clip(y, np.float32(0), np.float32(1)).astype(np.float64)
    if mode == 0:
        return unpack(yc), np.zeros((2 * h, 2 * w))
    K, sigma, lo, hi = np.float64(K), np.float64(sigma), np.float64(lo), np.float64(hi)
    z = yc * (hi - lo) + lo
    sg2 = (sigma / K) ** 2
    if mode == 2:
        pos = z > 0
        zp = z if defect == 'no_z_guard' else np.where(pos, z, 1.0)
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            t = ((zp / 2) ** 2, (1 / 4) * ((3 / 2) ** 0.5) * zp ** (-1.0), -(11 / 8) * zp ** (-2.0), (5 / 8) * ((3 / 2) ** 0.5) * zp ** (-3.0),
                 np.full(z.shape, -1 / 8), np.full(z.shape, -sg2))
            fz = t[0] + t[1] + t[2] + t[3] + t[4] + t[5]
            mag = sum(np.abs(v) for v in t)
        if defect != 'no_z_guard':
            fz, mag = np.where(pos, fz, 0.0), np.where(pos, mag, 0.0)
    else:
        fz = (z / 2) ** 2 - 3.0 / 8.0 - sg2
        mag = (z / 2) ** 2 + 3.0 / 8.0 + sg2
    band = 8 * 2.0 ** -53 * mag * K / scale
    with np.errstate(invalid='ignore'):
        raw = fz * K / scale
        band = np.where(raw < -band, 0.0, band)                    # max(fz, 0): firmly negative -> exactly 0
        r = np.maximum(fz, 0) * K / scale
        if clip01:
            band = np.where(raw > 1 + band, 0.0, band)
            r = np.clip(r, 0, 1)
    return unpack(r), unpack(band)


# ---------------------------------------------------------------------------------------------------------------------------
# N1
# ---------------------------------------------------------------------------------------------------------------------------
def gauss11():
    """cv2.getGaussianKernel(11, 1.5): exp(-(i - 5)^2 / (2 * 1.5^2)), normalised by the sum."""
    i = np.arange(11) - 5.0
    g = np.exp(-(i * i) / (2 * 1.5 * 1.5))
    return g / g.sum()


def ssim_map_ref(a, b, defect=None):
    """The SSIM map over the 'valid' positions of two float32 images in data range 1 (YOND_SIDD.py:652, 679-697)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if defect == 'x255_f64':
        A, B = a.astype(np.float64) * 255.0, b.astype(np.float64) * 255.0
    else:
        A, B = (a * np.float32(255.0)).astype(np.float64), (b * np.float32(255.0)).astype(np.float64)
    H, W = A.shape
    if defect == 'mask_le':                                       # one more row and column of windows, hanging over the edge into zeros
        A, B = np.pad(A, ((0, 1), (0, 1))), np.pad(B, ((0, 1), (0, 1)))
        H, W = H + 1, W + 1
    vh, vw = H - 10, W - 10
    g = gauss11()
    win = np.outer(g, g)
    Q = np.stack((A, B, A * A, B * B, A * B))                       # the five moments' integrands
    acc = np.zeros((5, vh, vw))
    tmp = np.empty((5, vh, vw))
    for dy in range(11):
        for dx in range(11):
            np.multiply(Q[:, dy:dy + vh, dx:dx + vw], win[dy, dx], out=tmp)
            acc += tmp
    m1, m2, e11, e22, e12 = acc
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    s1, s2, s12 = e11 - m1 * m1, e22 - m2 * m2, e12 - m1 * m2
    return ((2 * m1 * m2 + C1) * (2 * s12 + C2)) / ((m1 * m1 + m2 * m2 + C1) * (s1 + s2 + C2))


def ssim_ref(a, b, defect=None):
    """Mean SSIM over the 'valid' map (the divisor is the true number of valid positions whatever the defect)."""
    H, W = np.shape(a)
    return float(ssim_map_ref(a, b, defect).sum() / ((H - 10) * (W - 10)))


def se_ref(a, b, defect=None):
    """Sum of squared error in float64.  defect 'se_42': summed over the 42 x 42 input patch of every 32 x 32 tile (overlaps count twice)."""
    d = (np.asarray(a, np.float32).astype(np.float64) - np.asarray(b, np.float32).astype(np.float64)) ** 2
    if defect == 'se_42':
        H, W = d.shape
        return float(sum(d[y:y + 42, x:x + 42].sum() for y in range(0, H, 32) for x in range(0, W, 32)))
    return float(d.sum())


def psnr_ref(a, b, defect=None):
    """skimage peak_signal_noise_ratio with data_range 1: 10 log10(1 / mean((a - b)^2)); inf for identical images."""
    H, W = np.shape(a)
    mse = se_ref(a, b, defect) / (H * W)
    return float('inf') if mse == 0 else float(10 * np.log10(1.0 / mse))


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
def lo_hi(K, sigma, scale=SCALE):
    return float(vst64(0.0, K, sigma)), float(vst64(scale, K, sigma))


def preimage(target, scale=SCALE):
    """A float32 q with float32(q * float32(scale)) == float32(target), or None."""
    t, s = np.float32(target), np.float32(scale)
    q = np.float32(t / s)
    for _ in range(16):
        p = np.float32(q * s)
        if p == t:
            return q
        q = np.nextafter(q, np.float32(np.inf if p < t else -np.inf), dtype=np.float32)
    return None


def knot_hits(knots, scale=SCALE):
    """Pixels whose float32 product with scale lands exactly on a knot, and on the nearest float32 below and above it that a product
    can reach (where the product's binade is finer than the pixel's, every second float32 has no preimage): one or two ulp away."""
    out = []
    for t in knots:
        t32 = np.float32(t)
        if np.float64(t32) != np.float64(t):
            continue                                              # (not a float32 value: no pixel lands on it)
        q = preimage(t32, scale)
        if q is not None:
            out.append(q)
        for toward in ((np.inf, 0.0) if t32 > 0 else (np.inf,)):
            c = t32
            for _ in range(3):
                c = np.nextafter(c, np.float32(toward), dtype=np.float32)
                q = preimage(c, scale)
                if q is not None:
                    out.append(q)
                    break
    return out


# geometry: (name, H, W, (pad_l, pad_r, pad_t, pad_b))
K1_GEOMS = (
    ("2x2 no pad", 2, 2, (0, 0, 0, 0)),
    ("four pads", 40, 56, (3, 5, 2, 7)),
    ("largest pads", 12, 20, (9, 9, 5, 5)),
    ("Wp 255", 8, 500, (2, 3, 1, 0)),
    ("Wp 256", 8, 500, (3, 3, 0, 1)),
    ("Wp 257", 8, 500, (3, 4, 1, 1)),
    ("Wp 511", 6, 1000, (5, 6, 0, 0)),
    ("Wp 512", 6, 1000, (6, 6, 2, 0)),
    ("Wp 513", 6, 1000, (6, 7, 0, 2)),
    ("Wp 769", 4, 1530, (2, 2, 1, 1)),
    ("Hp 1", 2, 66, (4, 1, 0, 0)),
)
K1_MAIN = ("main", 96, 136, (6, 4, 5, 3))
K1_TOPS = (0.04, 0.3, 1.0)            # frame maxima (x scale 959: below 50, between 50 and 500, above 500 -> one, two, three runs of knots)
# (B, H, W, pads): Hp = 50, 47 and 50, B * Hp > 1536 rows over 1536 workgroups.  With 2 rows per workgroup the frames of Hp = 50 start on a
# workgroup's first row; Hp = 47 (2 rows each) and B = 70 (3 rows each) put frame starts in the middle of a workgroup's range.
K1_BATCH = ((40, 88, 24, (1, 1, 3, 3)), (33, 82, 28, (2, 0, 2, 4)), (70, 88, 24, (0, 1, 3, 3)))


def batch_crossings(B, Hp, wgs=1536):
    """Frames whose first row is not the first row of a workgroup's contiguous range (ceil(B Hp / wgs) rows per workgroup)."""
    per = -(-(B * Hp) // wgs)
    return sum(1 for b in range(1, B) if (b * Hp) % per != 0)


def k1_cases():
    """(name, H, W, pads, K, sigma, bc, top, seed); bc: False (no bias correction), True (get_bias' LUT for the frame's maximum),
    'synthetic' (get_bias' knots with synthetic_ordinates), '2d' (a merged row of the 2-D table of tests/golden/biaslut.npz).
    Every (K, sigma) with and without the bias correction on the main geometry at the three maxima, every geometry at a well- and an
    ill-conditioned pair, frames above the white point, synthetic ordinates and the 2-D table's three regimes."""
    out = []
    seed = 0
    for (K, s) in KSIG:
        for bc in (True, False):
            for top in (K1_TOPS if (K, s) in ((4.37, 6.27), (1.0, 400.0)) else (1.0,)):
                seed += 1
                out.append((f"{K1_MAIN[0]} K={K} s={s} bc={int(bc)} top={top}", K1_MAIN[1], K1_MAIN[2], K1_MAIN[3], K, s, bc, top, seed))
    for (K, s) in ((0.72, 1.8), (1.0, 400.0)):
        for gi, (gname, H, W, pads) in enumerate(K1_GEOMS):
            seed += 1
            out.append((f"{gname} K={K} s={s}", H, W, pads, K, s, True, K1_TOPS[gi % 3], seed))
    for (K, s) in ((4.37, 6.27), (1.0, 400.0)):
        for top in K1_TOPS:
            seed += 1
            out.append((f"synthetic LUT K={K} s={s} top={top}", K1_MAIN[1], K1_MAIN[2], K1_MAIN[3], K, s, 'synthetic', top, seed))
    for (K, s) in ((0.05, 0.3), (0.72, 1.8), (4.37, 6.27), (120.0, 0.0)):
        seed += 1
        out.append((f"2-D LUT K={K} s={s}", K1_MAIN[1], K1_MAIN[2], K1_MAIN[3], K, s, '2d', 1.0, seed))
    seed += 2
    out.append((f"above white K=4.37 s=6.27", K1_MAIN[1], K1_MAIN[2], K1_MAIN[3], 4.37, 6.27, True, 1.3, seed + 1))
    out.append((f"above white K=22.65 s=37.09 no bias", K1_MAIN[1], K1_MAIN[2], K1_MAIN[3], 22.65, 37.09, False, 1.3, seed + 2))
    return out


def k1_frame_base(H, W, K, sigma, top, seed, scale=SCALE):
    """The frame before the knot hits go in: uniform pixels up to `top` (one pixel exactly at top), negative pixels from just below zero
    down past the point where K x + 3/8 K^2 + sigma^2 turns negative, exact zeros and float32 subnormals.  Special values take < 1 %."""
    rng = np.random.default_rng(1000 + seed)
    f = (rng.random((H, W)) * top).astype(np.float32)
    f = np.minimum(f, np.float32(top))
    flat = f.reshape(-1)
    n = flat.size
    xz = -((3 / 8) * K ** 2 + sigma ** 2) / K / scale             # the pixel at which the VST's argument is zero
    neg = np.concatenate((xz * np.array([1e-6, 1e-3, 0.1, 0.5, 0.999, 1.0, 1.001, 1.5, 4.0]), [-1e-7, -1e-3 / scale, -1.0 / scale]))
    spec = np.concatenate((neg, [0.0, -0.0, 1e-45, 1e-40, 1.1754944e-38, 3e-39])).astype(np.float32)
    k = min(len(spec), max(n // 4 - 1, 0))                        # (a 2 x 2 frame takes none: its four pixels stay ordinary)
    pos = (np.arange(k) * 2 + 1) % n if n >= 16 else np.arange(k)
    flat[pos] = spec[:k]
    flat[n - 1] = np.float32(top)
    return f


def k1_frame(H, W, K, sigma, top, seed, lut_x=None, scale=SCALE):
    """k1_frame_base plus pixels exactly on knots of lut_x and one float32 ulp to either side (first, last, the repeated knots 50 and 500
    and their neighbours, the knots around each and a spread of others), as far as they fit below the frame's maximum."""
    f = k1_frame_base(H, W, K, sigma, top, seed, scale)
    if lut_x is None:
        return f
    flat = f.reshape(-1)
    n = flat.size
    mx = np.float32(np.float32(top) * np.float32(scale))
    lx = np.asarray(lut_x, np.float64)
    pick = [0.0, 0.1, 0.2, 49.9, 50.0, 51.0, 52.0, 499.0, 500.0]
    pick += [float(v) for v in lx[lx > 500.0][:2]] + [float(v) for v in lx[::97]] + [float(v) for v in lx[-3:]]
    hits = [q for q in knot_hits([t for t in pick if t <= float(mx)], scale) if np.float32(q * np.float32(scale)) <= mx]
    room = max(n // 100, 2) if n >= 64 else 0
    hits = hits[:room]
    if hits:
        start = n // 2
        flat[start:start + len(hits)] = np.array(hits, np.float32)
    return f


def bias_knots(ub):
    """utils/isp_algos.py:101-108: get_bias' grid for ub = ceil(max) + 1 -- runs of step 0.1 / 1 / ~10 joined by np.concatenate, so 50 and
    500 appear twice.  A float32 ub gives float32 knots in the run that ends at ub (NumPy 2): pass np.float32 or np.float64."""
    lb = 0
    if ub < 50:
        return np.linspace(lb, ub, int((ub - lb) / 0.1) + 2)
    if ub < 500:
        return np.concatenate((np.linspace(lb, 50, int((50 - lb) / 0.1) + 1), np.linspace(50, ub, int(ub - 50) + 2)))
    return np.concatenate((np.linspace(lb, 50, int((50 - lb) / 0.1) + 1), np.linspace(50, 500, 451), np.linspace(500, ub, int(ub - 500) // 10 + 2)))


def synthetic_ordinates(lx):
    """float32 ordinates with slopes that change at every knot and a JUMP between the two copies of a repeated knot: only
    searchsorted 'left' (the first copy's ordinate for a query equal to the knot) evaluates such a table as interp1d does."""
    lx = np.asarray(lx, np.float64)
    y = 0.2 * np.sin(lx / 40.0) + 0.05 * np.cos(lx * 3.0)
    second = np.concatenate(([False], lx[1:] == lx[:-1]))
    return (y + 0.01 * np.cumsum(second)).astype(np.float32)


def merged_row(table, x_lut, sg_lut, K, sigma):
    """BiasLUT.get_lut's sigma merge (utils/isp_algos.py:179-194, 199, 225): (knots in DN, merged float64 row), or None when sigma / K
    lies beyond the table's sigma grid."""
    sg_lut = np.asarray(sg_lut, np.float64)
    data = np.concatenate(([-np.inf], sg_lut))
    sg = np.float64(sigma) / np.float64(K)
    idx = int(np.searchsorted(data, sg).clip(0, len(data) - 1))
    with np.errstate(invalid='ignore'):
        pos = idx - (data[idx] - sg) / (data[idx] - data[idx - 1]) - 1
    if pos > len(sg_lut) - 1:
        return None
    pos = np.clip(pos, 0, len(x_lut) - 1)
    l, r = int(np.floor(pos)), int(np.ceil(pos))
    tab = np.asarray(table, np.float64).reshape(-1, len(sg_lut))
    return np.asarray(x_lut, np.float64) * np.float64(K), tab[:, l] * (1 - (pos - l)) + tab[:, r] * (pos - l)


def frame_max_dn(f, scale=SCALE):
    """What the pipeline hands to get_bias: the float32 maximum of the scaled frame."""
    return np.float32((np.asarray(f, np.float32) * np.float32(scale)).max())


# K4: (name, Hp, Wp, pad_t, pad_l, h, w)
K4_GEOMS = (
    ("interior crop", 20, 40, 2, 3, 15, 30),
    ("crop to the far edges", 20, 40, 5, 7, 15, 33),
    ("zero pads", 9, 31, 0, 0, 9, 31),
    ("w 1", 7, 5, 1, 2, 5, 1),
    ("w 255", 6, 260, 1, 5, 4, 255),
    ("w 256", 6, 256, 0, 0, 6, 256),
    ("w 257", 5, 259, 1, 1, 4, 257),
)
K4_BATCH = (70, 64, 24, 2, 3, 60, 20)             # (B, Hp, Wp, pad_t, pad_l, h, w): B * h = 4200 > 4096, the grid-stride path


def closed_form_zero(K, sigma):
    """The largest zero of z^2/4 + a/z - b/z^2 + c/z^3 - 1/8 - (sigma/K)^2 (bisection on [1, 50]: negative at 1, positive at 50)."""
    sg2 = (sigma / K) ** 2
    f = lambda z: (z / 2) ** 2 + 0.25 * 1.5 ** 0.5 / z - 1.375 / z ** 2 + 0.625 * 1.5 ** 0.5 / z ** 3 - 0.125 - sg2
    a, b = 1.0, 50.0
    assert f(a) < 0 < f(b)
    for _ in range(200):
        m = 0.5 * (a + b)
        a, b = (m, b) if f(m) < 0 else (a, m)
    return b


def k4_case_input(case):
    name, (gname, Hp, Wp, pt, pl, h, w), mode, clip, K, s, lo, hi, zmin, seed = case
    return k4_input(Hp, Wp, lo, hi, seed, zmin, closed_form_zero(K, s) if zmin is not None else None)


def k4_input(Hp, Wp, lo, hi, seed, zmin=None, zcross=None):
    """Network outputs in [0, 1) with a few in [-0.1, 0) and (1, 1.2] and exact 0 and 1, and -- zmin given -- values whose z = y (hi - lo) + lo is
    spread logarithmically from zmin up to hi (the closed form's steep small-z end) plus the inputs next to its zero crossing zcross."""
    rng = np.random.default_rng(2000 + seed)
    y = rng.random((Hp, Wp, 4))
    if zmin is not None:
        m = rng.random((Hp, Wp, 4)) < 0.5
        z = np.exp(rng.uniform(np.log(zmin), np.log(hi), (Hp, Wp, 4)))
        y = np.where(m, (z - lo) / (hi - lo), y)
    # below 0 and above 1: few, because every one of them is the same point of the curve (z = lo: the algebraic inverse cancels to
    # nothing there, so both neighbours of ~0 are admissible and the share would count them all)
    out = rng.random((Hp, Wp, 4))
    y = np.where(out < 0.004, -0.1 * rng.random((Hp, Wp, 4)), np.where(out > 0.996, 1.0 + 0.2 * rng.random((Hp, Wp, 4)), y))
    y = y.astype(np.float32)
    flat = y.reshape(-1)
    sp = [0.0, 1.0, -0.0, 0.5, 1e-45, 1.0000001, -1e-30, 0.99999994]
    if zcross is not None:
        # the float32 inputs on either side of the closed form's zero crossing: the terms cancel to nothing there
        q = np.float32((zcross - lo) / (hi - lo))
        up = dn = q
        sp.append(q)
        for _ in range(12):
            up, dn = np.nextafter(up, np.float32(2)), np.nextafter(dn, np.float32(-1))
            sp += [up, dn]
    sp = np.array(sp, np.float32)
    k = min(len(sp), flat.size)
    # (spread over the tensor so that a crop keeps most of them)
    pos = (np.arange(k) * (flat.size // k)) if k else np.arange(0)
    flat[pos] = sp[:k]
    return y


def k4_cases():
    """(name, geometry, mode, clip01, K, sigma, lo, hi, zmin, seed)"""
    out = []
    seed = 0
    for (K, s) in KSIG:
        lo, hi = lo_hi(K, s)
        for mode in (1, 2):
            for clip in (0, 1):
                seed += 1
                out.append((f"K={K} s={s} mode {mode} clip {clip}", K4_GEOMS[seed % 2], mode, clip, K, s, lo, hi, None, seed))
    for gi, g in enumerate(K4_GEOMS):
        seed += 1
        K, s = KSIG[2 + gi % 2]
        out.append((f"{g[0]} mode 2", g, 2, gi % 2, K, s) + lo_hi(K, s) + (None, seed))
    for (K, s) in ((4.37, 6.27), (0.72, 1.8), (120.0, 0.0)):
        seed += 1
        out.append((f"z 1e-3..50 K={K} s={s}", K4_GEOMS[0], 2, 0, K, s, 1e-3, 50.0, 1e-3, seed))
        seed += 1
        out.append((f"z -50..50 K={K} s={s}", K4_GEOMS[1], 2, 1, K, s, -50.0, 50.0, None, seed))
    out.append(("z -50..50 mode 1", K4_GEOMS[0], 1, 0, 4.37, 6.27, -50.0, 50.0, None, seed + 1))
    out.append(("mode 0", K4_GEOMS[0], 0, 0, 1.0, 0.0, 0.0, 1.0, None, seed + 2))
    out.append(("mode 0 far edges", K4_GEOMS[1], 0, 1, 1.0, 0.0, 0.0, 1.0, None, seed + 3))
    return out


# N1: (name, H, W, bh, bw)
N1_GEOMS = (
    ("11x11", 11, 11, 11, 11), ("11x300", 11, 300, 11, 300), ("12x43", 12, 43, 12, 43), ("32x32", 32, 32, 32, 32),
    ("33x42", 33, 42, 33, 42), ("74x75", 74, 75, 74, 75), ("100x90 in 300x270", 300, 270, 100, 90), ("256x256", 256, 512, 256, 256),
    ("whole 250x314", 250, 314, 250, 314),
)
N1_PAIRS = ('identical', 'const0', 'const1', 'const.5', 'const vs noise', 'inverted', 'independent', 'step on tile edge', 'step on valid edge', 'near')


def n1_pair(kind, H, W, bh, bw, seed=0):
    rng = np.random.default_rng(3000 + seed)
    hr = rng.random((H, W)).astype(np.float32)
    if kind == 'identical':
        return hr.copy(), hr
    if kind.startswith('const') and kind != 'const vs noise':
        c = np.float32({'const0': 0.0, 'const1': 1.0, 'const.5': 0.5}[kind])
        return np.full((H, W), c, np.float32), np.full((H, W), c, np.float32)
    if kind == 'const vs noise':
        return np.full((H, W), np.float32(0.25), np.float32), hr
    if kind == 'inverted':
        return (np.float32(1.0) - hr).astype(np.float32), hr
    if kind == 'independent':
        return rng.random((H, W)).astype(np.float32), hr
    if kind.startswith('step'):
        # a vertical and a horizontal step inside every block: at the 32-pixel tile boundary, or where the 'valid' map ends
        ey = min(32, bh - 1) if kind == 'step on tile edge' else bh - 10
        ex = min(32, bw - 1) if kind == 'step on tile edge' else bw - 10
        yy, xx = np.mgrid[0:H, 0:W]
        st = (((yy % bh) >= ey).astype(np.float32) * np.float32(0.5) + ((xx % bw) >= ex).astype(np.float32) * np.float32(0.25))
        hr = (st + np.float32(0.1) * hr).astype(np.float32)
        dn = (hr + np.float32(0.05) * rng.standard_normal((H, W)).astype(np.float32)).astype(np.float32)
        return dn, hr
    dn = np.clip(hr + np.float32(0.01) * rng.standard_normal((H, W)).astype(np.float32), 0, 1).astype(np.float32)
    return dn, hr


def blocks(a, bh, bw):
    H, W = a.shape
    return [a[y:y + bh, x:x + bw] for y in range(0, H, bh) for x in range(0, W, bw)]
