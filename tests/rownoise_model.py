"""TEST INFRASTRUCTURE ONLY -- the float64 model of the row-noise removal (include/yond_hip.h M5; the reference's utils/isp_algos.py:319-334
row_denoise), its single-defect variants, the restated 1-D bilateral filter that tools/gen_golden_rownoise.py hands the reference in
place of the absent cv2, the seeded frames of tests/golden/rownoise.npz, and the bounds the GPU tests use.

    p = y & 1, j = y >> 1, n = H / 2, r = d / 2
    per 'row':    m_p[j]     = (sums[y][0] + sums[y][1]) / W          sums[y][c]: the sum of in[y][x] over x % 2 == c, by math.fsum
    per 'plane':  m_{p,c}[j] = sums[y][c] / (W / 2)
    w_k    = exp(-k^2 / (2 ss^2)) * exp(-(m[jk] - m[j])^2 / (2 sc^2)),  jk = clamp(j + k, 0, n - 1),  k = -r .. r
    offset = m[j] - sum_k w_k m[jk] / sum_k w_k,  evaluated as  sum_k w_k (m[j] - m[jk]) / sum_k w_k
    out    = float32(float64(in) - offset[y][x & 1])

The second form of the offset is the same quantity: equal means give exactly 0 in it (d = 1, or one row per parity), and its rounding
error scales with the differences between the means instead of their level.  `cv2_bilateral_1d` is the first, literal form; the two
differ by about d * 2^-53 * level (1.4e-12 at level 500), far inside the fixture's 1e-9.

Containment (this project's, not the reference's): a neighbour whose mean is not finite has weight 0; a row whose own mean is not finite
has offset 0; a pixel whose offset is 0 is copied, bit for bit.

THE BOUNDS, with u = 2^-53.

Stage 1, the sums.  n float64 additions in ANY order are within (n - 1) u sum |x| of the exact sum to first order (each partial sum is
rounded once, and is at most sum |x|); a column phase of a row has W / 2 terms:  |sums_gpu - fsum| <= (W / 2) u sum_c |x|.

Stage 2, the offsets from given sums.  The means are IEEE additions and divisions of the same numbers on both sides: equal bits.  So
are the differences dlt_k = m[j] - m[jk] and both arguments of exp.  What differs:
  * exp.  The device's is the ROCm device library's (OCML), which implements OpenCL C's math functions; the OpenCL C specification
    ("Relative error as ULPs") allows exp 3 ulp in double precision.  (HIP's own table of math functions lists a smaller figure; the
    specification's is used.)  The host's is NumPy's, within 1 ulp (glibc's documented bound for exp; NumPy's SIMD loops claim less).
    One ulp is at most 2^-52 = 2 u relative: a factor differs by at most 4 ulp = 8 u between the sides, a weight (two factors, one
    product rounded on either side) by e_w = 2 * 8 u + 2 u = 18 u.  A weight below the smallest normal number may be flushed or lose
    bits on either side: an absolute 2.3e-308 per tap, carried below.
  * the products w_k dlt_k, one rounding a side (2 u), and the two sums of d terms in different orders ((d - 1) u sum |terms| a side).
  With A = sum_k w_k |dlt_k| and D = sum_k w_k (D >= 1: tap 0 has weight 1):  |N_gpu - N_model| <= (e_w + 2 u + 2 (d - 1) u) A,
  |D_gpu - D_model| <= (e_w + 2 (d - 1) u) D, the quotient is rounded on either side (2 u), and |N| <= A, so to first order
      |offset_gpu - offset_model| <= (2 e_w + 4 d u) A / D = (36 + 4 d) u * A / D   (+ d * 2.3e-308 * max |dlt_k|)
  `offset_band` returns it per value; A / D is the weighted mean of |dlt_k|, at most the largest difference in the window.  At d = 25
  and A / D = 3 that is 4.5e-14.

Stage 3, the output from given offsets: one float64 subtraction of exact operands and one conversion, both IEEE: bit for bit.

Stage 4, end to end.  The sums differ by stage 1's bound (fsum's own rounding adds u |s|), a mean by
      eta = (ds_0 + ds_1) / W + 4 u |m|  ('row';  'plane': ds_c / (W / 2) + 4 u |m|)
  (one addition and one division rounded on either side).  A difference dlt_k moves by at most 2 eta_max, eta_max the largest eta in
  the window.  offset = N / D with dw_k / d dlt_k = -w_k dlt_k / sc^2:
      |d offset / d dlt_k| <= w_k (1 + dlt_k^2 / sc^2 + |offset| |dlt_k| / sc^2) / D =: S_k,      |offset_gpu - offset_model| <= 2 eta_max sum_k S_k
  to first order (eta / sc is below 1e-8 at every shape tested: the second order is below 1e-8 of the first, a factor 1 + 1e-6 covers
  it), plus stage 2's band.  `e2e_band` returns the sum; the float32 result is within half an ulp of its float64 value, so
      |out_gpu - (float64(in) - offset_model)| <= ulp32(out_gpu) / 2 + e2e_band.
"""
import math

import numpy as np

ROW, PLANE = 'row', 'plane'
U = 2.0 ** -53
DEFECTS = ('no_parity', 'reflect_border', 'no_range_weight', 'radius_d', 'row_mean_half_width', 'plane_swapped', 'offset_added', 'nan_spreads')


def cv2_bilateral_1d(src, d, sigmaColor, sigmaSpace, borderType=None):
    """cv2.bilateralFilter restated from its documentation for a 1 x n image (OpenCV is absent: UNPINNED): radius d / 2, weights Gaussian
    in distance and in value, the result normalised, the border replicated.  Literal form, sequential float64 sums; the input's dtype is
    kept.  (OpenCV's window is a disc: on a 1 x n image a real cv2 also visits the replicated rows above and below, which gives tap k a
    further factor sum over |dy| <= sqrt(r^2 - k^2) of exp(-dy^2 / (2 sigmaSpace^2)).  That factor is NOT restated here.)"""
    a = np.asarray(src)
    v = a.astype(np.float64).reshape(-1)
    n, r = v.size, int(d) // 2
    out = np.empty(n, np.float64)
    for j in range(n):
        num = den = 0.0
        for k in range(-r, r + 1):
            vk = v[min(max(j + k, 0), n - 1)]
            w = math.exp(-(k * k) / (2.0 * sigmaSpace * sigmaSpace)) * math.exp(-((vk - v[j]) ** 2) / (2.0 * sigmaColor * sigmaColor))
            num += w * vk
            den += w
        out[j] = num / den
    return out.reshape(a.shape).astype(a.dtype)


def _fsum(a):
    a = np.asarray(a, np.float64).reshape(-1)
    if not np.isfinite(a).all():
        with np.errstate(invalid='ignore'):
            return float(a.sum())                            # NaN or an infinity, as any order of additions gives
    return math.fsum(a.tolist())


def row_sums(x):
    """float64 [H][2]: the correctly rounded sums of the two column phases of every row."""
    x = np.asarray(x)
    return np.array([[_fsum(row[0::2]), _fsum(row[1::2])] for row in x], np.float64).reshape(x.shape[0], 2)


def means_of(sums, W, per, defect=None):
    """float64 [H][2]: the mean of the sequence that (row y, column phase c) belongs to."""
    sums = np.asarray(sums, np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        if per == ROW:
            m = (sums[:, 0] + sums[:, 1]) / np.float64(W // 2 if defect == 'row_mean_half_width' else W)
            return np.stack([m, m], axis=1)
        return sums / np.float64(W if defect == 'row_mean_half_width' else W // 2)


def _filter(m, d, sc, ss, defect=None):
    """(offset, A / D, sum_k S_k) of one sequence m[0..n-1], each float64 [n]."""
    n = m.size
    r = int(d) if defect == 'radius_d' else int(d) // 2
    two_sc2, two_ss2 = 2.0 * sc * sc, 2.0 * ss * ss
    j = np.arange(n)
    num, den, a_sum, s_sum = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    taps = []
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        for k in range(-r, r + 1):
            if defect == 'reflect_border' and n > 1:
                jk = np.abs(j + k) % (2 * (n - 1))
                jk = np.where(jk > n - 1, 2 * (n - 1) - jk, jk)
            else:
                jk = np.clip(j + k, 0, n - 1)
            mk = m[jk]
            dlt = m - mk
            wr = np.ones(n) if defect == 'no_range_weight' else np.exp(-(dlt * dlt) / two_sc2)
            w = np.exp(-np.float64(k * k) / two_ss2) * wr
            if defect != 'nan_spreads':
                fin = np.isfinite(mk)
                w, dlt = np.where(fin, w, 0.0), np.where(fin, dlt, 0.0)
            num += w * dlt
            den += w
            taps.append((w, dlt))
        off = num / den
        if defect != 'nan_spreads':
            off = np.where(np.isfinite(m), off, 0.0)
        for w, dlt in taps:
            a_sum += w * np.abs(dlt)
            s_sum += w * (1.0 + dlt * dlt / (sc * sc) + np.abs(off) * np.abs(dlt) / (sc * sc))
        own = np.isfinite(m)                                 # (a row without a finite mean: offset 0, nothing to bound)
        return off, np.where(own, a_sum / den, 0.0), np.where(own, s_sum / den, 0.0)


def offsets_from_sums(sums, W, per=ROW, d=25, sc=10.0, ss=9.0, defect=None, detail=False):
    """float64 [H][2] offsets of a frame whose row sums are `sums`; with detail also A / D and sum_k S_k of the docstring, [H][2] each."""
    m = means_of(sums, W, per, defect)
    H = m.shape[0]
    out = [np.zeros((H, 2)) for _ in range(3)]
    for c in range(2):
        if defect == 'no_parity':
            res = _filter(m[:, c], d, sc, ss)
            for o, v in zip(out, res):
                o[:, c] = v
        else:
            for p in range(2):
                res = _filter(m[p::2, c], d, sc, ss, defect)
                for o, v in zip(out, res):
                    o[p::2, c] = v
    if defect == 'plane_swapped' and per == PLANE:
        out = [o[:, ::-1].copy() for o in out]
    return tuple(out) if detail else out[0]


def apply(x, offsets, defect=None):
    """(float32 out, float64 value before the one rounding): in - offset[y][x & 1]; a pixel whose offset is 0 is copied."""
    x = np.asarray(x, np.float32)
    off = np.empty(x.shape, np.float64)
    off[:, 0::2], off[:, 1::2] = offsets[:, 0:1], offsets[:, 1:2]
    with np.errstate(invalid='ignore', over='ignore'):
        z = x.astype(np.float64) + off if defect == 'offset_added' else x.astype(np.float64) - off
        out = np.where(off == 0, x, z.astype(np.float32)).astype(np.float32)
    return out, z


def row_denoise(x, per=ROW, d=25, sc=10.0, ss=9.0, defect=None, sums=None):
    """(out float32, offsets float64 [H][2], float64 values before rounding) of one frame."""
    x = np.asarray(x)
    sums = row_sums(x) if sums is None else sums
    offsets = offsets_from_sums(sums, x.shape[1], per, d, sc, ss, defect)
    out, z = apply(x, offsets, defect)
    return out, offsets, z


def row_denoise_f64(x, iso, defect=None):
    """The reference's call on a float64 frame, all in float64 (no float32 rounding of the result): sigma_color 10, sigma_space
    1 + iso / 200, d 25, per sensor row."""
    x = np.asarray(x, np.float64)
    offsets = offsets_from_sums(row_sums(x), x.shape[1], ROW, 25, 10.0, 1.0 + iso / 200.0, defect)
    off = np.repeat(offsets[:, :1], x.shape[1], axis=1)
    with np.errstate(invalid='ignore'):
        return x + off if defect == 'offset_added' else x - off


# ---- bounds (derived in the module docstring) ------------------------------------------------------------------------------------------

def sums_bound(x):
    """float64 [H][2]: (W / 2) u sum_c |x| per entry."""
    ax = np.abs(np.asarray(x, np.float64))
    W = ax.shape[1]
    return (W // 2) * U * np.array([[_fsum(row[0::2]), _fsum(row[1::2])] for row in ax]).reshape(ax.shape[0], 2)


def offset_band(sums, W, per, d, sc, ss):
    """float64 [H][2]: stage 2's band (36 + 4 d) u A / D + d * 2.3e-308 * (the largest |dlt| a window can hold)."""
    _, a_over_d, _ = offsets_from_sums(sums, W, per, d, sc, ss, detail=True)
    m = means_of(sums, W, per)
    fin = m[np.isfinite(m)]
    spread = float(fin.max() - fin.min()) if fin.size else 0.0
    return (36.0 + 4.0 * d) * U * a_over_d + d * 2.3e-308 * spread


def e2e_band(x, per, d, sc, ss):
    """float64 [H][2]: stage 4's band on the offsets, 2 eta_max sum_k S_k (1 + 1e-6) + stage 2's, with the model's own sums."""
    x = np.asarray(x)
    H, W = x.shape
    sums, ds = row_sums(x), sums_bound(x)
    with np.errstate(invalid='ignore'):
        ds = ds + U * np.abs(sums)
        m = means_of(sums, W, per)
        if per == ROW:
            eta = np.repeat(((ds[:, 0] + ds[:, 1]) / W)[:, None], 2, axis=1) + 4 * U * np.abs(m)
        else:
            eta = ds / (W // 2) + 4 * U * np.abs(m)
    eta = np.where(np.isfinite(eta), eta, 0.0)               # (a row without a finite mean has weight 0 everywhere)
    r, n = d // 2, H // 2
    eta_max = np.zeros((H, 2))
    for p in range(2):
        e = eta[p::2]
        for j in range(n):
            eta_max[2 * j + p] = e[max(j - r, 0):j + r + 1].max(axis=0)
    _, _, s_sum = offsets_from_sums(sums, W, per, d, sc, ss, detail=True)
    return 2.0 * eta_max * s_sum * (1.0 + 1e-6) + offset_band(sums, W, per, d, sc, ss)


def per_pixel(band, W):
    """[H][2] -> [H][W]."""
    out = np.empty((band.shape[0], W), np.float64)
    out[:, 0::2], out[:, 1::2] = band[:, 0:1], band[:, 1:2]
    return out


# ---- seeded frames ---------------------------------------------------------------------------------------------------------------------

def frame(seed, H, W, step=0.0, heavy=False, sig_row=3.0, sig_plane=1.0, sig_pix=5.0, level=500.0):
    """float64 [H][W], a function of its arguments alone: a level with a gentle ramp down the rows, one offset per sensor row (sig_row), one
    per row of a CFA plane (sig_plane), white noise (sig_pix); `step` is added to the lower half (an edge across rows); heavy: every
    value times 10^U(-3, 3)."""
    rng = np.random.RandomState(seed)
    y = np.arange(H, dtype=np.float64)[:, None]
    x = level + 4.0 * y / H + rng.normal(0.0, sig_row, (H, 1)) + np.zeros((1, W))
    plane = rng.normal(0.0, sig_plane, (H, 2))
    x[:, 0::2] += plane[:, 0:1]
    x[:, 1::2] += plane[:, 1:2]
    x += rng.normal(0.0, sig_pix, (H, W))
    x[H // 2:] += step
    if heavy:
        x *= 10.0 ** rng.uniform(-3.0, 3.0, (H, W))
    return x


GOLDEN = {                   # name -> (seed, H, W, frame keywords, dtype handed to the reference, iso)
    'g1_60x96': (31, 60, 96, {}, np.float64, 1600),
    'g2_step_52x16': (32, 52, 16, {'step': 80.0}, np.float64, 800),
    'g3_f32_12x16': (33, 12, 16, {}, np.float32, 1600),
    'g4_10x8': (34, 10, 8, {}, np.float64, 6400),
    'g5_nan_60x16': (35, 60, 16, {}, np.float64, 1600),
}
GOLDEN_NAN_AT = (9, 5)       # g5: one NaN pixel (the reference has no containment: its odd rows up to 9 + 24 are NaN)


def golden_frame(name):
    seed, H, W, kw, dtype, iso = GOLDEN[name]
    x = frame(seed, H, W, **kw).astype(dtype)
    if 'nan' in name:
        x[GOLDEN_NAN_AT] = np.nan
    return x, iso
