"""Float64 models of the training step's small kernels (csrc/train.hip) with per-element error bounds, float32 restatements of the
kernels' own steps, single-defect variants, and the operand generators of tests/test_train_model.py and tests/test_hip_train_edges.py.
Plain NumPy, independent of the library.

Every model returns (value, bound): the float64 value of the operation on the float32 operands it is given, and a bound on
|kernel - value| per output element.  The bounds are DERIVED from the kernels' rounding steps (the derivation stands beside each formula)
and are sums of absolute terms -- never a multiple of the largest element, so a quiet channel is held as tightly as a loud one.

Notation.  E = 2^-24: the relative error of one float32 rounding (round to nearest).  A float32 operation whose result is subnormal is off
by up to TINY = 2^-149 absolutely instead; every bound carries a few TINY.  The library is built with -ffp-contract=off: no operation is
fused unless the source says so, so "one rounding per operation" counts the operations of the source.  Division and square root are
correctly rounded (hipcc's default).  expf is ASSUMED to be within EXPF_ULP = 2 ulp (the HIP math documentation is not at hand; the OCML
figure is 1 ulp): relative error X = EXPF_ULP * 2 E.  A float32 sum of L terms added in any order is off by at most
gamma(L - 1) * sum |term|, gamma(k) = k E / (1 - k E); float atomics arrive in any order, so L counts every addition a term can pass.
"""
import math

import numpy as np

E = 2.0 ** -24
TINY = 2.0 ** -149
EXPF_ULP = 2.0
X = EXPF_ULP * 2.0 * E
# expf(-u) overflows to +inf below u = -88.7228...: the kernels' sigmoid is then exactly 0 and SiLU / SiLU' return -0 where the true value
# is u e^u (1 + ...) -- at most 88.73 e^-88.72 = 2.6e-37 in magnitude.  Every SiLU bound carries this absolute floor.
EXPF_OVERFLOW = 88.72283935546875           # float32 neighbour below ln(FLT_MAX) = 88.72283905...
SILU_FLOOR = 3.0e-37


def gamma(k):
    k = np.maximum(np.asarray(k, np.float64), 0.0)
    return k * E / (1.0 - k * E)


def f32(a):
    return np.asarray(a, np.float32)


def f64(a):
    return np.asarray(a, np.float64)


def ratio(got, ref, bound):
    """Worst |got - ref| / bound; an element with bound 0 must be hit exactly (ratio 0 or inf).  NaN anywhere -> inf."""
    err = np.abs(f64(got) - f64(ref))
    bound = f64(bound)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0.0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# Adam (adam_kernel, adam_dev_kernel)
# ---------------------------------------------------------------------------------------------------------------------------
def adam_hyp(lr, b1, t, b2):
    """The step's two scalars as train.TrainStep._hyp forms them (Python doubles)."""
    return lr / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t)


def adam_model(p, g, m, v, lr, b1, b2, eps, t):
    """One Adam step in float64 on float32 state; hyperparameters are the Python doubles.  Returns ((p', m', v'), (bp, bm, bv)).

      m' = m + (1-b1)(g-m)        roundings: g-m, the constant float32(1-b1), the product, the sum:
                                    bm = E (3 |(1-b1)(g-m)| + |m'|)                        <= E (|m| + 4 (1-b1) |g-m|)
      v' = b2 v + (1-b2) g^2      roundings: the constants b2 and 1-b2, v b2, g g, (g g)(1-b2), the sum:
                                    bv = E (2 b2 v + 3 (1-b2) g^2 + v')                    =  E (3 b2 v + 4 (1-b2) g^2)
      p' = p - step q, q = m' / d, d = sqrt(v') ibc2 + eps
           sqrt of an operand off by bv:  ds = min(bv / sqrt(v'), sqrt(bv))   (|sqrt a - sqrt b| <= |a-b| / max(sqrt a, sqrt b) and <= sqrt|a-b|)
           roundings: sqrt, the constant ibc2, the product, the constant eps, the sum:
                                    bd = ds ibc2 + E (3 sqrt(v') ibc2 + eps + d)           <= ds ibc2 + E (4 sqrt(v') ibc2 + 2 eps)
           quotient of operands off by bm, bd, one rounding:  bq = (bm + |q| bd) / (d - bd) + E |q|
           roundings: the constant step, the product, the difference:  bp = step bq + E (2 |step q| + |p'|)  <= step bq + E (|p| + 3 |step q|)
    Each line carries a few TINY for results in the subnormal range."""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    step, ibc2 = adam_hyp(lr, b1, t, b2)
    o1, o2 = 1.0 - b1, 1.0 - b2
    m1 = m + o1 * (g - m)
    bm = E * (np.abs(m) + 4.0 * o1 * np.abs(g - m)) + 3 * TINY
    v1 = b2 * v + o2 * g * g
    bv = E * (3.0 * b2 * v + 4.0 * o2 * g * g) + 4 * TINY
    s = np.sqrt(v1)
    with np.errstate(divide='ignore'):
        ds = np.minimum(bv / s, np.sqrt(bv))
    d = s * ibc2 + eps
    bd = ds * ibc2 * (1 + 4 * E) + E * (4.0 * s * ibc2 + 2.0 * eps) + 3 * TINY
    q = m1 / d
    bq = (bm + np.abs(q) * bd) / (d - bd) + E * np.abs(q) + TINY
    p1 = p - step * q
    bp = step * bq * (1 + 2 * E) + E * (np.abs(p) + 3.0 * np.abs(step * q)) + 2 * TINY
    return (p1, m1, v1), (bp, bm, bv)


def adam_f32(p, g, m, v, lr, b1, b2, eps, t, defect=None, order='kernel'):
    """The kernels' steps in float32 NumPy, one rounding per operation.  defect: None, 'omb_f32' (the complements formed as 1.0f - float32(beta):
    the library before this model existed), 'no_bc1' (lr in place of lr / (1 - b1^t)).
    order 'torch': the two state lines as torch's CPU kernels round them -- lerp_ is ONE fused multiply-add, m' = fma(w1, g - m, m), and
    addcmul_ multiplies the scalar first and fuses the rest, v' = fma(w2 g, g, v b2) -- restated through float64 (a product of two float32
    values is exact there).  Same constants, same operations, a rounding of one product apart from the kernels' unfused order."""
    p, g, m, v = f32(p), f32(g), f32(m), f32(v)
    step, ibc2 = adam_hyp(lr, b1, t, b2)
    if defect == 'no_bc1':
        step = lr
    o1, o2 = np.float32(1.0 - b1), np.float32(1.0 - b2)
    if defect == 'omb_f32':
        o1, o2 = np.float32(1.0) - np.float32(b1), np.float32(1.0) - np.float32(b2)
    if order == 'torch':
        m1 = (f64(m) + f64(o1) * f64(g - m)).astype(np.float32)
        v1 = (f64(v * np.float32(b2)) + f64(o2 * g) * f64(g)).astype(np.float32)
    else:
        m1 = m + o1 * (g - m)
        v1 = v * np.float32(b2) + (g * g) * o2
    d = np.sqrt(v1) * np.float32(ibc2) + np.float32(eps)
    p1 = p - np.float32(step) * (m1 / d)
    return p1, m1, v1


def adam_operands(n, kind, seed=0):
    """(p, g, m, v) float32.  'heavy': g spans 1e-12 .. 1e3 (log-uniform, random sign), exact zeros of g where v = 0 and m = 0 (the
    denominator is eps alone), a tenth of v subnormal.  'first': the first step's state, m = v = 0."""
    r = np.random.default_rng(1000 + seed + n % 9973)
    g = (10.0 ** r.uniform(-12, 3, n) * r.choice([-1.0, 1.0], n)).astype(np.float32)
    p = r.standard_normal(n).astype(np.float32)
    if kind == 'first':
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        m = (g.astype(np.float64) * r.uniform(-1, 1, n)).astype(np.float32)
        v = (g.astype(np.float64) ** 2 * 10.0 ** r.uniform(-2, 1, n)).astype(np.float32)
        sub = np.arange(n) % 10 == 3
        v[sub] = (r.integers(1, 1 << 20, int(sub.sum())) * TINY).astype(np.float32)         # subnormal second moments
    z = np.arange(n) % 7 == 2
    g[z], m[z], v[z] = 0.0, 0.0, 0.0
    return p, g, m, v


# ---------------------------------------------------------------------------------------------------------------------------
# losses (l1_kernel, charbonnier_kernel)
# ---------------------------------------------------------------------------------------------------------------------------
def l1_model(pred, target):
    """(loss_sum, bound), grad.  d = float32(pred - target) is the kernel's own first step and exact input of both outputs.  The kernel adds
    |d| in float64 in its own order: n additions of non-negative terms, bound n 2^-53 sum.  grad = sign(d) float32(1 / n), 0 at d == +-0,
    exact (1.0f / (float)n is one correctly rounded division; n < 2^24 converts exactly)."""
    d = f32(pred) - f32(target)
    n = d.size
    s = float(np.sum(np.abs(d.astype(np.float64))))
    gs = np.float32(1.0) / np.float32(n)
    grad = np.where(d > 0, gs, np.where(d < 0, -gs, np.float32(0.0))).astype(np.float32)
    return (s, n * 2.0 ** -53 * s), grad


def charbonnier_f32(pred, target, eps, fused=False):
    """The float32 steps charbonnier_kernel names: d, e = sqrt(d d + eps), gu = (1/n) / (2 e), t = gu d, grad = t + t.  Returns (e, grad).
    fused: the defect grad = (2 gu) d -- the same number unless gu d is subnormal."""
    d = f32(pred) - f32(target)
    n = d.size
    e = np.sqrt(d * d + np.float32(eps))
    gu = (np.float32(1.0) / np.float32(n)) / (np.float32(2.0) * e)
    if fused:
        return e, (np.float32(2.0) * gu) * d
    t = gu * d
    return e, t + t


def charbonnier_model(pred, target, eps):
    """(loss_sum, bound), (grad64, band).  The loss is the float64 sum of the kernel's float32 e (reordering only, as L1).  The gradient
    d / sqrt(d^2 + eps) / n in float64 on the float32 d; the kernel's value carries the roundings of d d, eps, the sum (halved by the
    square root: 1.5 E), the root, 1/n, the quotient, gu d (2 e and t + t are exact): 5.5 E relative, stated as 6 E, plus TINY."""
    e, _ = charbonnier_f32(pred, target, eps)
    d = (f32(pred) - f32(target)).astype(np.float64)
    n = d.size
    s = float(np.sum(e.astype(np.float64)))
    g = d / np.sqrt(d * d + eps) / n
    return (s, n * 2.0 ** -53 * s), (g, 6.0 * E * np.abs(g) + 2 * TINY)


def loss_operands(n, seed=0):
    """pred, target in [0, 1] with runs of pred == target (one element in five, in runs of up to 8), some differences of -0.0's kind (both
    zero with opposite signs) and some subnormal differences."""
    r = np.random.default_rng(2000 + seed + n % 9973)
    t = r.uniform(0, 1, n).astype(np.float32)
    p = (t + r.standard_normal(n).astype(np.float32) * np.float32(0.05)).astype(np.float32)
    run = (np.arange(n) // 8) % 5 == 1
    p[run] = t[run]
    i = np.arange(n)
    p[i % 31 == 5], t[i % 31 == 5] = -0.0, 0.0                                # d = -0.0
    s = i % 37 == 11
    t[s] = 0.0
    p[s] = (r.integers(1, 1 << 12, int(s.sum())) * TINY).astype(np.float32)   # subnormal d
    return p, t


# ---------------------------------------------------------------------------------------------------------------------------
# colsum (colsum_kernel, colsum_wide_kernel)
# ---------------------------------------------------------------------------------------------------------------------------
def colsum_geometry(npix, C):
    """The launcher's choice: ('main', nb, ppw) -- workgroup b takes the pixels p with (p // ppw) % nb == b -- or ('wide', gy, 8)."""
    c4 = C // 4
    if C <= 256 and 256 % c4 == 0:
        ppw = 256 // c4
        return 'main', max(1, min(1024, -(-npix // (ppw * 8)))), ppw
    return 'wide', min(256, -(-npix // 512)), 8


def colsum_partials(dy, nb, ppw):
    """[nb][C] float64: each workgroup's sum (pixel p belongs to workgroup (p // ppw) % nb)."""
    dy = f32(dy)
    npix, C = dy.shape
    per = nb * ppw
    full = npix // per
    part = np.zeros((nb, C), np.float64)
    if full:
        part += dy[:full * per].reshape(full, nb, ppw, C).sum(axis=(0, 2), dtype=np.float64)
    if npix > full * per:
        pad = np.zeros((per, C), np.float32)
        pad[:npix - full * per] = dy[full * per:]
        part += pad.reshape(nb, ppw, C).sum(axis=1, dtype=np.float64)
    return part


def colsum_model(dy):
    """(db64 [C], bound [C]).  A thread adds its pixels in float64 (k terms), the workgroup adds the threads' sums in float64: an error of
    at most (k + ppw) 2^-53 sum |dy|, kept though negligible.  Each workgroup's partial is rounded to float32 once -- E |partial| -- and
    the nb partials meet in float32 atomics in any order: gamma(nb - 1) sum_b |partial_b|.  The bound follows |partial| per workgroup,
    not |dy| per pixel: offsets that cancel inside a workgroup cost nothing, an all-zero channel has bound 0."""
    dy32 = f32(dy)
    npix, C = dy32.shape
    _, nb, ppw = colsum_geometry(npix, C)
    part = colsum_partials(dy32, nb, ppw)
    ref = dy32.sum(axis=0, dtype=np.float64)
    sa = np.abs(part).sum(axis=0)
    k = -(-npix // (nb * ppw))
    bound = (E + gamma(nb - 1)) * sa * (1 + E) + (k + ppw) * 2.0 ** -53 * np.abs(dy32).sum(axis=0, dtype=np.float64)
    bound = bound + np.where(sa > 0, TINY, 0.0)
    return ref, bound


def colsum_sim(dy, seed=0, defect=None):
    """Structure-faithful simulation: float64 per thread and workgroup, float32 partials, float32 atomics in a random order.
    defect: 'f32_threads' (float32 thread accumulators), 'drop_tail' (the pixel the two-in-flight loop leaves for its tail is skipped)."""
    dy32 = f32(dy)
    npix, C = dy32.shape
    kind, nb, ppw = colsum_geometry(npix, C)
    if defect is None:
        # (no [k][nb][ppw][C] array: the workgroups' float64 sums directly, then their float32 roundings and the float32 atomics)
        part = colsum_partials(dy32, nb, ppw).astype(np.float32)
        db = np.zeros(C, np.float32)
        for b in np.random.default_rng(seed).permutation(nb):
            db = db + part[b]
        return db
    per = nb * ppw
    k = -(-npix // per)
    acc_t = np.float32 if defect == 'f32_threads' else np.float64
    pad = np.zeros((k * per, C), np.float32)
    pad[:npix] = dy32
    pad = pad.reshape(k, nb, ppw, C)
    if defect == 'drop_tail':
        # a thread takes its pixels in pairs (p, p + stride); one whose count is odd takes the last in the tail `if (p < npix)`
        cnt = (np.arange(k * per).reshape(k, nb, ppw) < npix).sum(axis=0)
        bb, pp = np.nonzero(cnt % 2 == 1)
        pad[cnt[bb, pp] - 1, bb, pp, :] = 0.0
    thr = np.zeros((nb, ppw, C), acc_t)
    for j in range(k):
        thr = (thr + pad[j].astype(acc_t)).astype(acc_t)
    part = thr.astype(np.float64).sum(axis=1).astype(np.float32)         # [nb][C]
    order = np.random.default_rng(seed).permutation(nb)
    db = np.zeros(C, np.float32)
    for b in order:
        db = db + part[b]
    return db


def colsum_operands(npix, C, seed=0):
    """dy [npix][C] float32: O(1) noise on per-channel offsets of +-1e4 whose sign alternates with the pixel (the last pixel of an odd
    count has none), so that every channel's sum is O(sqrt(npix)) while a thread -- which sees pixels of one parity only: its stride is
    even -- holds sums of 1e4 k.  Channel 5 is all zero; channels 0 and 1 carry no offset."""
    r = np.random.default_rng(3000 + seed + C)
    base = r.standard_normal((min(npix, 4099), C)).astype(np.float32)
    dy = np.resize(base, (npix, C)).copy() if npix > base.shape[0] else base
    off = (r.choice([-1.0, 1.0], C) * 1e4).astype(np.float32)
    off[:2] = 0.0
    sign = np.where(np.arange(npix) % 2 == 0, 1.0, -1.0).astype(np.float32)
    if npix % 2:
        sign[-1] = 0.0
    dy = dy + sign[:, None] * off[None, :]
    dy[:, 5] = 0.0
    return np.ascontiguousarray(dy, np.float32)


def colsum_npix(C):
    kind, _, ppw = colsum_geometry(1 << 30, C)
    if kind == 'main':
        return [1, 7, 8 * ppw - 1, 8 * ppw + 1, 1024 * 8 * ppw + 3 * ppw + 1]
    return [1, 7, 8 * 64 - 1, 8 * 64 + 1, 256 * 8 * 64 + 3 * 8 + 1]


# ---------------------------------------------------------------------------------------------------------------------------
# SiLU, SiLU' (silu_f, dsilu_f), silu_kernel, silu_bwd_add_kernel
# ---------------------------------------------------------------------------------------------------------------------------
def sigmoid64(u):
    u = f64(u)
    e = np.exp(-np.abs(u))
    return np.where(u >= 0, 1.0, e) / (1.0 + e)


def silu_eval(u, du=0.0):
    """SiLU(u) = u s in float64 and the bound of the kernel's u / (1 + expf(-u)) evaluated at a float32 u' with |u' - u| <= du.
    Given u': e = expf(-u') is off by X relative, so 1 + e by X e / (1 + e) = X (1 - s); the sum and the quotient round once each:
    |SiLU| (2 E + X (1 - s)).  The operand's error passes through |SiLU'| <= 1.1 and |SiLU''| <= 0.5: du (|SiLU'(u)| + du / 2).
    SILU_FLOOR covers expf's overflow and quotients in the subnormal range."""
    u = f64(u)
    s = sigmoid64(u)
    val = u * s
    d1 = s * (1.0 + u * (1.0 - s))
    bound = np.abs(val) * (2 * E + X * (1.0 - s)) + du * (np.abs(d1) + 0.5 * du) + SILU_FLOOR
    return val, bound


def dsilu_eval(u, du=0.0):
    """SiLU'(u) = s (1 + u (1 - s)) and the bound of dsilu_f's steps at a float32 u' within du of u:
       s' = 1 / (1 + expf(-u')): ds = s (2 E + X (1 - s));  a = 1 - s: da = ds + E a;  b = u a: db = |u| da + E |u| a;
       c = 1 + b: dc = db + E |c|;  D = s c: dD = ds |c| + s dc + E |D|.
    The derivative crosses zero near u = -1.278 by cancellation in c, so the bound is E-sized multiples of s and s |u| (1 - s) and not
    relative to the result.  The operand's error passes through SiLU'' = s (1 - s) (2 + u (1 - 2 s)) and |SiLU'''| <= 0.5."""
    u = f64(u)
    s = sigmoid64(u)
    a = 1.0 - s
    c = 1.0 + u * a
    val = s * c
    ds = s * (2 * E + X * a)
    da = ds + E * a
    db = np.abs(u) * da + E * np.abs(u) * a
    dc = db + E * np.abs(c)
    dD = (ds * np.abs(c) + s * dc + E * np.abs(val)) * (1 + 8 * E)
    d2 = s * a * (2.0 + u * (1.0 - 2.0 * s))
    bound = dD + du * (np.abs(d2) + 0.5 * du) + SILU_FLOOR
    return val, bound


def silu_f32(u):
    """silu_f in float32 NumPy (np.exp on float32 is within 1 ulp)."""
    u = f32(u)
    with np.errstate(over='ignore'):
        return u / (np.float32(1.0) + np.exp(-u))


def dsilu_f32(u, defect=None):
    """dsilu_f in float32 NumPy.  defect 'no_u_term': s alone (the u (1 - s) term dropped)."""
    u = f32(u)
    with np.errstate(over='ignore'):
        s = np.float32(1.0) / (np.float32(1.0) + np.exp(-u))
    if defect == 'no_u_term':
        return s
    return s * (np.float32(1.0) + u * (np.float32(1.0) - s))


def silu_model(x):
    return silu_eval(f32(x))


def silu_bwd_add_model(x, dz, dres):
    """dx = dres + dz SiLU'(x): |dz| dD, the product's and the sum's roundings E (|dz D| + |dx|) <= E (|dres| + 2 |dz D|)."""
    D, dD = dsilu_eval(f32(x))
    g, r = f64(f32(dz)), f64(f32(dres))
    val = r + g * D
    bound = np.abs(g) * dD + E * (np.abs(r) + 2.0 * np.abs(g * D)) + 2 * TINY
    return val, bound


def silu_operands(n, seed=0):
    """u over [-120, 120] -- 99 % uniform over [-88, 88], 1 % over the whole range, so that about 0.13 % lie below the expf-overflow point --
    with both float32 neighbours of +-88.72 (and of the overflow point itself), +-0 and subnormals in front and at the end."""
    r = np.random.default_rng(4000 + seed + n % 9973)
    u = np.where(r.uniform(0, 1, n) < 0.01, r.uniform(-120, 120, n), r.uniform(-88, 88, n)).astype(np.float32)
    t = np.float32(EXPF_OVERFLOW)
    a = np.float32(88.72)
    sp = [np.nextafter(a, np.float32(0)), a, np.nextafter(a, np.float32(200)), np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(200))]
    sp = sp + [-q for q in sp] + [0.0, -0.0, TINY, -TINY, 2.0 ** -127, -2.0 ** -130, -1.2784645, 1.0, -1.0]
    sp = np.asarray(sp, np.float32)
    k = min(n, sp.size)
    u[:k] = sp[:k]
    if n > 64:
        u[-sp.size:] = sp                                          # ... and in the last elements (the tail of the grid-stride loop)
    return u


def floor_share(u):
    """Share of the elements at or below the expf-overflow point, where the kernels return -0 and SILU_FLOOR is all that holds them.  No
    check excludes them (the floor is a term of their bound).  The operand generators keep the share of the DRAWN values below 1 %;
    silu_operands also plants the overflow point's own float32 neighbours -- two of them at or below it, in front and again at the end --
    so its small cases exceed 1 % by exactly those (4 / 256 = 1.6 %).  The tests print the share."""
    return float(np.mean(f64(u) <= -EXPF_OVERFLOW))


# ---------------------------------------------------------------------------------------------------------------------------
# FiLM + SiLU (film_silu_fwd_kernel, film_silu_bwd_kernel)
# ---------------------------------------------------------------------------------------------------------------------------
def film_silu_geometry(N, P, C, bwd):
    """(nb, ppw): workgroups per image and pixels per workgroup pass, as the launchers choose them."""
    cap = 2048 // N + 1
    if bwd:
        ppw = 256 // (C // 4)
        return min(cap, -(-P // (ppw * 8))), ppw
    return min(cap, -(-(P * (C // 4)) // 2048)), 0


def _film_u(z, tk, tb):
    """u = z tk + tb in float64 and du, the float32 evaluation's error: the product and the sum round once, E (|z tk| + |u|)."""
    z, tk, tb = f64(f32(z)), f64(f32(tk))[:, None, :], f64(f32(tb))[:, None, :]
    u = z * tk + tb
    return u, E * (np.abs(z * tk) + np.abs(u)) + 2 * TINY


def film_silu_fwd_model(z, tk, tb):
    """z [N][P][C], tk, tb [N][C] -> (out, bound) per element."""
    u, du = _film_u(z, tk, tb)
    return silu_eval(u, du)


def film_silu_bwd_model(z, tk, tb, dout, launch_N=None):
    """-> dict of (value, bound) for dz [N][P][C], dtk, dtb [N][C].  launch_N: the batch size of the launch when z holds only some of its
    images (the grid's cap depends on it; the images are independent otherwise).
       g = dout D(u):  bg = |dout| dD + E |g|;   dz = g tk: bz = |tk| bg + E |dz|.
       dtb = sum_p g, dtk = sum_p g z: a term is off by bg resp. |z| bg + E |g z| (the product), and passes at most L - 1 float32
       additions: k in its thread (k = pixels per thread), ppw in the workgroup's LDS sum, nb - 1 atomics (only workgroups that own pixels add
       a nonzero): gamma(k + ppw + nb - 1) sum_p |term|."""
    zz = f64(f32(z))
    N, P, C = zz.shape
    u, du = _film_u(z, tk, tb)
    D, dD = dsilu_eval(u, du)
    go = f64(f32(dout))
    g = go * D
    bg = np.abs(go) * dD + E * np.abs(g) + TINY
    k64 = f64(f32(tk))[:, None, :]
    dz = g * k64
    bz = np.abs(k64) * bg + E * np.abs(dz) + TINY
    nb, ppw = film_silu_geometry(launch_N or N, P, C, True)
    nbe = min(nb, -(-P // ppw))
    k = -(-P // (nb * ppw))
    G = gamma(k + ppw + nbe - 1) * (1 + E)
    gz = g * zz
    dtb = g.sum(axis=1)
    btb = bg.sum(axis=1) + G * (np.abs(g) + bg).sum(axis=1) + TINY
    dtk = gz.sum(axis=1)
    bgz = np.abs(zz) * bg + E * np.abs(gz) + TINY
    btk = bgz.sum(axis=1) + G * (np.abs(gz) + bgz).sum(axis=1) + TINY
    return {'dz': (dz, bz), 'dtk': (dtk, btk), 'dtb': (dtb, btb)}


def film_silu_sim(z, tk, tb, dout, defect=None, seed=0):
    """Structure-faithful float32 simulation of both kernels: (out, dz, dtk, dtb).  Threads add their pixels in float32 in order, the
    workgroup adds its ppw rows in float32, the workgroups' partials meet in a random order.  defect 'dtk_sum_g': dtk sums g, not g z."""
    z, tk, tb, dout = f32(z), f32(tk), f32(tb), f32(dout)
    N, P, C = z.shape
    u = z * tk[:, None, :] + tb[:, None, :]
    out = silu_f32(u)
    g = dout * dsilu_f32(u)
    dz = g * tk[:, None, :]
    nb, ppw = film_silu_geometry(N, P, C, True)
    per = nb * ppw
    k = -(-P // per)
    rng = np.random.default_rng(seed)

    def reduce(term):
        pad = np.zeros((N, k * per, C), np.float32)
        pad[:, :P] = term
        pad = pad.reshape(N, k, nb, ppw, C)
        thr = np.zeros((N, nb, ppw, C), np.float32)
        for j in range(k):
            thr = thr + pad[:, j]
        wg = np.zeros((N, nb, C), np.float32)
        for r in range(ppw):
            wg = wg + thr[:, :, r]
        tot = np.zeros((N, C), np.float32)
        for b in rng.permutation(nb):
            tot = tot + wg[:, b]
        return tot
    return out, dz, reduce(g if defect == 'dtk_sum_g' else g * z), reduce(g)


def film_silu_operands(N, P, C, seed=0):
    """z, tk, tb, dout float32 with u = z tk + tb over [-100, 100] but only about 0.5 % of it below the expf-overflow point: z is normal,
    tk log-uniform over 0.05 .. 30 with random sign and tb normal with deviation 3 (|u| > 88.7 needs |z| > 2.8 at the largest |tk|).
    Channels 3 and 17 have tk = 0 (dz = 0 exactly); dout carries per-channel scales 1e-4 .. 1e2."""
    r = np.random.default_rng(5000 + seed + 7 * C + P + N)
    z = r.standard_normal((N, P, C)).astype(np.float32)
    tk = (10.0 ** r.uniform(np.log10(0.05), np.log10(30.0), (N, C)) * r.choice([-1.0, 1.0], (N, C))).astype(np.float32)
    tk[:, [3, 17]] = 0.0
    tb = (3.0 * r.standard_normal((N, C))).astype(np.float32)
    scale = (10.0 ** r.uniform(-4, 2, C)).astype(np.float32)
    dout = (r.standard_normal((N, P, C)) * scale).astype(np.float32)
    u = z * tk[:, None, :] + tb[:, None, :]
    z = np.where(np.abs(u) > 100.0, np.float32(0.0), z).astype(np.float32)
    return z, tk, tb, dout


# ---------------------------------------------------------------------------------------------------------------------------
# zero_interleave
# ---------------------------------------------------------------------------------------------------------------------------
def zero_interleave_model(dy, H, W, defect=None):
    """dy [N][Ho][Wo][C] -> g [N][H][W][C], exact.  defect 'floor_ho': the source rows indexed with Ho = H // 2 (wrong on odd H)."""
    dy = f32(dy)
    N, Ho, Wo, C = dy.shape
    assert Ho == (H + 1) // 2 and Wo == (W + 1) // 2
    g = np.zeros((N, H, W, C), np.float32)
    if defect == 'floor_ho':
        flat = dy.reshape(-1, C)
        ho = H // 2
        for n in range(N):
            for y in range(0, H, 2):
                for x in range(0, W, 2):
                    i = (n * ho + y // 2) * Wo + x // 2
                    g[n, y, x] = flat[i % flat.shape[0]]
        return g
    g[:, ::2, ::2] = dy
    return g


# ---------------------------------------------------------------------------------------------------------------------------
# the sigma MLPs of a guided block (film_mlp_tile_kernel modes 0..5, film_mlp_vec_kernel)
# ---------------------------------------------------------------------------------------------------------------------------
def _prod(A, dA, Bm, dB):
    """sum_k A[m][k] B[k][n] with operands off by dA, dB: every product rounds once and passes at most K float32 additions (the kernel adds
    K rounded up to 64 terms in order; the zero padding adds nothing): gamma(K) sum |A||B| (1 + ...) + sum (dA |B| + |A| dB + dA dB)."""
    A, Bm = f64(A), f64(Bm)
    K = A.shape[1]
    val = A @ Bm
    ab = np.abs(A) @ np.abs(Bm)
    op = dA @ np.abs(Bm) + np.abs(A) @ dB + dA @ dB
    return val, (gamma(K) + E) * (ab + op) + op + TINY


def _h(t, w1, b1):
    """a = t w1 + b1 [B][C] and its float32 evaluation's error."""
    t, w1, b1 = f64(f32(t))[:, None], f64(f32(w1))[None, :], f64(f32(b1))[None, :]
    a = t * w1 + b1
    return a, E * (np.abs(t * w1) + np.abs(a)) + 2 * TINY


def film_mlp_models(t, w1, b1, W2, b2, W3, b3, tk_dev=None, dtk=None, dtb=None, dtk_tot_dev=None, da_dev=None, defect=None):
    """Every stage of yond_film_mlp_fwd_f32 / _bwd_f32 as (value, bound), each from the float32 operands THAT stage reads: a later stage is
    modelled on the earlier stage's actual output (tk_dev, dtk_tot_dev, da_dev: what the kernels wrote), so every bound is one stage's.
    C = len(w1) real channels; tk_dev, dtk, dtb are [B][C] (the caller strips the padding).  Epilogues: + bias rounds once (E |out|);
    mode 2: dtk + acc SiLU'(tk): E (|acc D| + |out|) + |acc| dD + bacc |D|; mode 3: acc SiLU'(a): E |out| + |acc| dD + bacc |D|.
    defect 'mode2_no_dtk': the mode-2 epilogue without its dtk term."""
    W2, W3 = f64(f32(W2)), f64(f32(W3))
    out = {}
    a, da_ = _h(t, w1, b1)
    h, dh = silu_eval(a, da_)
    acc, bacc = _prod(h, dh, W2.T, np.zeros_like(W2.T))
    tk = acc + f64(f32(b2))[None, :]
    out['tk'] = (tk, bacc + E * np.abs(tk) + TINY)
    if tk_dev is None:
        return out
    tkd = f64(f32(tk_dev))
    s, dsv = silu_eval(tkd)
    acc, bacc = _prod(s, dsv, W3.T, np.zeros_like(W3.T))
    tb = acc + f64(f32(b3))[None, :]
    out['tb'] = (tb, bacc + E * np.abs(tb) + TINY)
    if dtk is None:
        return out
    dtk, dtb = f64(f32(dtk)), f64(f32(dtb))
    zero = lambda q: np.zeros_like(q)
    # mode 2
    acc, bacc = _prod(dtb, zero(dtb), W3, zero(W3))
    D, dD = dsilu_eval(tkd)
    v = (0.0 if defect == 'mode2_no_dtk' else dtk) + acc * D
    out['dtk_tot'] = (v, np.abs(acc) * dD + bacc * (np.abs(D) + dD) + E * (np.abs(acc * D) + np.abs(v)) + 2 * TINY)
    if dtk_tot_dev is None:
        return out
    dt = f64(f32(dtk_tot_dev))
    # mode 3
    acc, bacc = _prod(dt, zero(dt), W2, zero(W2))
    D, dD = dsilu_eval(a, da_)
    v = acc * D
    out['da'] = (v, np.abs(acc) * dD + bacc * (np.abs(D) + dD) + E * np.abs(v) + 2 * TINY)
    # modes 4, 5
    out['dW3'] = _prod(dtb.T, zero(dtb.T), s, dsv)
    out['dW2'] = _prod(dt.T, zero(dt.T), h, dh)
    # the vector sums: four partial sums of ceil(B / 4) terms in float32, joined by three additions: gamma(ceil(B / 4) + 2) sum |term|
    B = dt.shape[0]
    G = gamma(-(-B // 4) + 2)
    out['db3'] = (dtb.sum(0), G * np.abs(dtb).sum(0) + TINY)
    out['db2'] = (dt.sum(0), G * np.abs(dt).sum(0) + TINY)
    if da_dev is not None:
        dd = f64(f32(da_dev))
        tt = f64(f32(t))[:, None]
        out['dw1'] = ((dd * tt).sum(0), (G + E) * np.abs(dd * tt).sum(0) * (1 + E) + TINY)
        out['db1'] = (dd.sum(0), G * np.abs(dd).sum(0) + TINY)
    return out


def film_mlp_sim(t, w1, b1, W2, b2, W3, b3, dtk, dtb):
    """The kernels' stages in float32 NumPy, products added in k order (float32 accumulator): dict of arrays named as film_mlp_models'."""
    t, w1, b1, W2, b2, W3, b3, dtk, dtb = (f32(q) for q in (t, w1, b1, W2, b2, W3, b3, dtk, dtb))

    def mm(A, Bm):
        acc = np.zeros((A.shape[0], Bm.shape[1]), np.float32)
        for k in range(A.shape[1]):
            acc = acc + A[:, k:k + 1] * Bm[k:k + 1, :]
        return acc
    a = t[:, None] * w1[None, :] + b1[None, :]
    h = silu_f32(a)
    tk = mm(h, W2.T) + b2[None, :]
    s = silu_f32(tk)
    tb = mm(s, W3.T) + b3[None, :]
    dtk_tot = dtk + mm(dtb, W3) * dsilu_f32(tk)
    da = mm(dtk_tot, W2) * dsilu_f32(a)
    return dict(tk=tk, tb=tb, dtk_tot=dtk_tot, da=da, dW3=mm(dtb.T, s), dW2=mm(dtk_tot.T, h), db3=dtb.sum(0, dtype=np.float32),
                db2=dtk_tot.sum(0, dtype=np.float32), dw1=(da * t[:, None]).sum(0, dtype=np.float32), db1=da.sum(0, dtype=np.float32))


def film_mlp_operands(B, C, seed=0):
    """Heavy-tailed operands (Student t, 3 degrees of freedom) at the scales of the network's MLPs."""
    r = np.random.default_rng(6000 + seed + 13 * B + C)
    ht = lambda *s: r.standard_t(3, s).astype(np.float32)
    t = (r.uniform(0.01, 0.31, B)).astype(np.float32)
    return dict(t=t, w1=ht(C) * 4, b1=ht(C) * np.float32(0.05), W2=ht(C, C) / np.float32(C ** 0.5), b2=ht(C) * np.float32(0.05) + 1,
                W3=ht(C, C) / np.float32(C ** 0.5), b3=ht(C) * np.float32(0.05), dtk=ht(B, C), dtb=ht(B, C))


# ---------------------------------------------------------------------------------------------------------------------------
# the case lists shared by the CPU and the GPU module
# ---------------------------------------------------------------------------------------------------------------------------
FLAT_SIZES = (1, 255, 256, 257)
ADAM_CAP = 1024 * 256 + 1                    # one element past the capped grid's single pass (Adam, the losses)
SILU_CAP = 4 * (4096 * 256) + 4              # the same for the SiLU pair (four floats per thread)
COLSUM_C = (32, 64, 128, 256, 96, 512, 1024)
FILM_C = (32, 256, 512, 1024)
ZI_CASES = ((1, 1, 1, 4), (3, 5, 7, 36), (2, 6, 9, 32))
MLP_B = (1, 17, 64)
MLP_C = ((8, 32), (24, 32), (96, 96), (512, 512))      # (C, padded row stride)


def film_P(C):
    ppw = 256 // (C // 4)
    return sorted({1, max(1, ppw - 1), ppw + 1, 97})
