"""Training-mode BatchNorm2d + ReLU (csrc/bn_train.hip, include/yond_hip.h "yond_bn_*") restated in NumPy: the exact float64 model, the
kernels' own arithmetic, and the per-element error bounds that follow from that arithmetic.  Imports no reference code.

Tensors are [M][C] float32 (an [N][H][W][C] tensor, M = N H W values per channel).

    exact(...)      float64: two-pass variance, no float32 rounding anywhere -- what the kernels approximate
    kernel(...)     the kernels' steps in their own precisions: float64 sums of y and y y (exact products), one float32 rounding each of
                    mean, rstd, scale, shift, dgamma, dbeta, the fused multiply-add of apply, the float32 chain of the backward apply
    bounds(...)     a priori bounds on |kernel - exact| for every output, term by term from those steps (u = 2^-24, v = 2^-53):
      sums          a float64 sum of M terms in ANY order is off by at most (M - 1) v sum|term|;  G = 2 (M + 8) v is used (the factor 2 also
                    covers this model's own float64 steps)
      mean          em = G S1 / M + v |mean|                                                   (S1 = sum |y|)
      var           ev = G S2 / M + 2 |mean| em + 4 v (S2 / M + mean^2)                         (S2 = sum y^2; Syy / M - mean^2)
      rstd          relative  er = ev / (2 (var + eps)) + 4 v
      out           the float64 pair gives (y - mean_c) scale_c + beta:  |y - mean| |scale| er + em |scale| + 2 v (|beta| + |mean scale|);
                    rounding scale and shift to float32 and the fma's one rounding add  u (|y scale| + |shift| + |pre-activation|)
      running       momentum em + u |rm'| + 4 v (|rm| + |mean|);   momentum ev M / (M - 1) + u |rv'| + 4 v (|rv| + var M / (M - 1))
      yh            (y - mean32) rstd32 in two float32 roundings:  eyh = (em + u |mean|) rstd + |yh| (er + 3 u)
      dbeta         G sum|g| + u |dbeta|;      dgamma   sum |g| eyh + G sum |g yh| + u |dgamma|
      dy            t1 = g - fl(dbeta / M):  e1 = edbeta / M + u |dbeta / M| + u |g - dbeta / M|
                    t  = fma(-yh, fl(dgamma / M), t1):  et = e1 + |yh| (edgamma / M + u |dgamma / M|) + |dgamma / M| eyh + u |t|
                    dy = scale32 t:  |scale| et + |t| |scale| (er + 2 u) + u |dy|
    Every bound carries a factor 1.001 for the second-order terms and one float32 subnormal (1.5e-45) for underflow.
The bounds are NOT fitted to any kernel output: tests/test_bn_model.py holds kernel(...) to them on the CPU, tests/test_hip_bn_train.py
the HIP kernels."""
import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
SLACK = 1.001
TINY = 1.5e-45
EPS_REFERENCE = 1e-4
MOMENTUM_REFERENCE = 0.95


def _f64(*a):
    return [np.asarray(t, np.float64) for t in a]


def exact(y, gamma, beta, rm, rv, eps=EPS_REFERENCE, momentum=MOMENTUM_REFERENCE):
    """Forward in float64.  Returns a dict: mean, var (biased), rstd, scale, shift, pre (pre-activation), out, rm_new, rv_new."""
    y, gamma, beta, rm, rv = _f64(y, gamma, beta, rm, rv)
    M = y.shape[0]
    mean = y.sum(0) / M
    var = ((y - mean) ** 2).sum(0) / M
    rstd = 1.0 / np.sqrt(var + eps)
    scale = gamma * rstd
    shift = beta - mean * scale
    pre = (y - mean) * scale + beta
    with np.errstate(invalid='ignore'):
        out = np.where(pre > 0, pre, np.where(pre <= 0, 0.0, pre))       # (a NaN stays a NaN, as torch's ReLU keeps it)
    return dict(mean=mean, var=var, rstd=rstd, scale=scale, shift=shift, pre=pre, out=out,
                rm_new=(1 - momentum) * rm + momentum * mean, rv_new=(1 - momentum) * rv + momentum * var * (M / (M - 1.0)))


def exact_backward(y, dout, mask, fwd):
    """Backward in float64 for a given ReLU mask ([M][C] bool).  Returns dict: g, yh, dbeta, dgamma, dy."""
    y, dout = _f64(y, dout)
    M = y.shape[0]
    g = np.where(mask, dout, 0.0)
    yh = (y - fwd['mean']) * fwd['rstd']
    dbeta, dgamma = g.sum(0), (g * yh).sum(0)
    dy = fwd['scale'] * (g - dbeta / M - yh * (dgamma / M))
    return dict(g=g, yh=yh, dbeta=dbeta, dgamma=dgamma, dy=dy)


def fmaf(a, b, c):
    """float32 fused multiply-add: the product of two float32 is exact in float64, the sum is rounded there and again to float32 (a
    double rounding that differs from a true fma only on a float64 tie next to a float32 tie: inside every bound here)."""
    with np.errstate(invalid='ignore', over='ignore'):
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def kernel(y, gamma, beta, rm, rv, eps=EPS_REFERENCE, momentum=MOMENTUM_REFERENCE):
    """The four forward outputs as the kernels form them.  Returns dict: stat [4][C] float32 (mean, rstd, scale, shift), pending [2][C]
    float32, out [M][C] float32."""
    y32 = np.asarray(y, np.float32)
    y, gamma, beta, rm, rv = _f64(y32, gamma, beta, rm, rv)
    M = y.shape[0]
    sy, syy = y.sum(0), (y * y).sum(0)
    mean = sy / M
    var = (syy - sy * mean) / M
    with np.errstate(invalid='ignore'):
        var = np.where(var < 0, 0.0, var)
    rstd = 1.0 / np.sqrt(var + eps)
    scale = gamma * rstd
    shift = beta - mean * scale
    stat = np.stack([mean, rstd, scale, shift]).astype(np.float32)
    pending = np.stack([(1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * (var * (M / (M - 1.0)))]).astype(np.float32)
    pre = fmaf(y32, stat[2], stat[3])
    with np.errstate(invalid='ignore'):
        out = np.where(pre > 0, pre, np.where(pre <= 0, np.float32(0), pre)).astype(np.float32)
    return dict(stat=stat, pending=pending, out=out, pre=pre)


def kernel_backward(y, dout, stat):
    """dgamma, dbeta [C] float32 and dy [M][C] float32 as the kernels form them (the mask recomputed from stat)."""
    y32, d32 = np.asarray(y, np.float32), np.asarray(dout, np.float32)
    M = y32.shape[0]
    mean, rstd, scale, shift = stat
    with np.errstate(invalid='ignore'):
        g = np.where(fmaf(y32, scale, shift) > 0, d32, np.float32(0)).astype(np.float32)
        yh = ((y32 - mean).astype(np.float32) * rstd).astype(np.float32)
        dbeta = g.astype(np.float64).sum(0).astype(np.float32)
        dgamma = (g.astype(np.float64) * yh.astype(np.float64)).sum(0).astype(np.float32)
        mg = (dgamma.astype(np.float64) / M).astype(np.float32)
        mb = (dbeta.astype(np.float64) / M).astype(np.float32)
        t = fmaf(-yh, mg, (g - mb).astype(np.float32))
        dy = (scale * t).astype(np.float32)
    return dict(dgamma=dgamma, dbeta=dbeta, dy=dy)


def _terms(y, fwd, eps):
    y = np.asarray(y, np.float64)
    M = y.shape[0]
    G = 2.0 * (M + 8) * U64
    S1, S2 = np.abs(y).sum(0), (y * y).sum(0)
    mean, var = fwd['mean'], fwd['var']
    em = G * S1 / M + U64 * np.abs(mean)
    ev = G * S2 / M + 2 * np.abs(mean) * em + 4 * U64 * (S2 / M + mean * mean)
    er = ev / (2 * (var + eps)) + 4 * U64
    return M, G, em, ev, er


def bounds(y, gamma, beta, rm, rv, fwd, eps=EPS_REFERENCE, momentum=MOMENTUM_REFERENCE):
    """Bounds on |kernel - exact| of the forward outputs.  fwd: exact(...).  Returns dict: mean, rstd, scale, shift, out, rm_new, rv_new."""
    y, gamma, beta, rm, rv = _f64(y, gamma, beta, rm, rv)
    M, G, em, ev, er = _terms(y, fwd, eps)
    mean, var, rstd, scale, shift, pre = (fwd[k] for k in ('mean', 'var', 'rstd', 'scale', 'shift', 'pre'))
    a = np.abs
    b = dict(
        mean=em + U32 * a(mean),
        rstd=rstd * (er + U32),
        scale=a(scale) * (er + 2 * U64 + U32),
        shift=em * a(scale) + a(mean * scale) * (er + 4 * U64) + 2 * U64 * (a(beta) + a(mean * scale)) + U32 * a(shift),
        out=(a(y - mean) * a(scale) * er + em * a(scale) + 2 * U64 * (a(beta) + a(mean * scale))
             + U32 * (a(y * scale) + a(shift) + a(pre))),
        rm_new=momentum * em + U32 * a(fwd['rm_new']) + 4 * U64 * (a(rm) + a(mean)),
        rv_new=momentum * ev * (M / (M - 1.0)) + U32 * a(fwd['rv_new']) + 4 * U64 * (a(rv) + var * (M / (M - 1.0))),
    )
    return {k: v * SLACK + TINY for k, v in b.items()}


def bounds_backward(y, fwd, bwd, eps=EPS_REFERENCE):
    """Bounds on |kernel - exact| of dbeta, dgamma [C] and dy [M][C].  bwd: exact_backward(...) on the SAME mask the kernel used."""
    y = np.asarray(y, np.float64)
    M, G, em, ev, er = _terms(y, fwd, eps)
    a = np.abs
    mean, rstd, scale = fwd['mean'], fwd['rstd'], fwd['scale']
    g, yh, dbeta, dgamma, dy = (bwd[k] for k in ('g', 'yh', 'dbeta', 'dgamma', 'dy'))
    eyh = (em + U32 * a(mean)) * rstd + a(yh) * (er + 3 * U32)
    edb = G * a(g).sum(0) + U32 * a(dbeta)
    edg = (a(g) * eyh).sum(0) + G * a(g * yh).sum(0) + U32 * a(dgamma)
    t1 = g - dbeta / M
    e1 = edb / M + U32 * a(dbeta / M) + U32 * a(t1)
    t = t1 - yh * (dgamma / M)
    et = e1 + a(yh) * (edg / M + U32 * a(dgamma / M)) + a(dgamma / M) * eyh + U32 * a(t)
    edy = a(scale) * et + a(t) * a(scale) * (er + 2 * U32) + U32 * a(dy)
    return dict(dbeta=edb * SLACK + TINY, dgamma=edg * SLACK + TINY, dy=edy * SLACK + TINY)


def worst_ratio(got, want, bound):
    """max |got - want| / bound over the finite elements (every element must be finite where `want` is)."""
    got, want, bound = _f64(got, want, bound)
    bound = np.broadcast_to(bound, want.shape)
    fin = np.isfinite(want)
    assert np.isfinite(got[fin]).all(), "non-finite output where the model is finite"
    if not fin.any():
        return 0.0
    return float((np.abs(got[fin] - want[fin]) / bound[fin]).max())


def make_case(name, C=32):
    """Seeded inputs of the named edge cases: (y [M][C], dout [M][C], gamma, beta, rm, rv) float32."""
    shapes = {'m2': (1, 1, 2), 'ragged': (3, 5, 7), 'multi': (2, 64, 64), 'constant': (1, 3, 5), 'cancel': (3, 5, 7), 'dead': (1, 4, 6),
              'boundary': (1, 3, 4), 'nan': (1, 4, 5)}
    N, H, W = shapes[name]
    M = N * H * W
    rng = np.random.default_rng([sum(map(ord, name)), C])
    y = (rng.standard_normal((M, C)) * rng.uniform(0.2, 3.0, C) + rng.standard_normal(C)).astype(np.float32)
    dout = rng.standard_normal((M, C)).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, C).astype(np.float32) * np.where(rng.random(C) < 0.25, -1, 1).astype(np.float32)
    beta = (rng.standard_normal(C) * 0.3).astype(np.float32)
    rm = (rng.standard_normal(C) * 0.1).astype(np.float32)
    rv = np.exp(rng.uniform(np.log(0.25), np.log(4.0), C)).astype(np.float32)
    if name == 'constant':                       # channel 3: every value the same -> var = 0, rstd = 100
        y[:, 3] = np.float32(0.7)
        beta[3] = np.float32(0.25)
    if name == 'cancel':                         # channel 5: mean 1e3, deviation 1e-2
        y[:, 5] = (1e3 + 1e-2 * rng.standard_normal(M)).astype(np.float32)
    if name == 'dead':                           # channel 1: gamma = 0, beta < 0; channel 2: shift far below every y scale
        gamma[1], beta[1] = np.float32(0), np.float32(-0.5)
        gamma[2], beta[2] = np.float32(1.0), np.float32(-1e3)
    if name == 'boundary':                       # channel 0: gamma = 1, beta = 0, values -1, +1 and zeros around a zero mean: with
        y[:, 0] = 0                              # eps > 0 the pre-activation of the zeros is exactly 0
        y[0, 0], y[1, 0] = np.float32(1), np.float32(-1)
        gamma[0], beta[0] = np.float32(1), np.float32(0)
    if name == 'nan':
        y[2, 7] = np.float32(np.nan)
    return y, dout, gamma, beta, rm, rv


CASE_NAMES = ('m2', 'ragged', 'multi', 'constant', 'cancel', 'dead', 'boundary', 'nan')
