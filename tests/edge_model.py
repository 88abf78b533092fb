"""Float64 models of the forward's edge layers and glue kernels (csrc/conv_misc.hip: conv_in, conv_out, maxpool2, film; csrc/estnet.hip:
est_conv_in, est_head; csrc/vst.hip: image_max and the layout copies) with per-element error bounds, float32 restatements of the kernels'
own steps, single-defect variants, and the operand generators and case tables of tests/test_edge_model.py and
tests/test_hip_edge_layers.py.  Plain NumPy, independent of the library.

Every bounded model returns (value, bound): the float64 value of the operation on the float32 operands it is given and a bound on
|kernel - value| per output element.  The bounds are DERIVED from the kernels' rounding steps (the derivation stands beside each formula)
and are sums of absolute terms -- never a multiple of the largest element, so a quiet channel is held as tightly as a loud one.

Notation as in tests/train_model.py: E = 2^-24 is the relative error of one float32 rounding, TINY = 2^-149 the absolute error of one whose
result is subnormal, gamma(k) = k E / (1 - k E) bounds a value that passes k roundings.  The library is built with -ffp-contract=off: the only
fusions are the fmaf calls and the MFMA of the source.  Division is correctly rounded, so the staged a = float32(x / ub) is an exact operand
of what follows and carries no bound term.  expf is assumed within EXPF_ULP ulp (train_model.silu_eval).

ASSUMPTION (conv_in only): an fp32 MFMA is a chain of fused multiply-adds, ONE rounding per k-step, and it keeps subnormals.  The CDNA
programming guide says so; nobody has measured it in this project.  Should conv_in alone exceed its bound on the GPU while the float32
restatement here does not, the admitted fallback is two roundings per step (an unfused multiply-add): CONV_IN_ROUNDINGS = 72.

A fused multiply-add is restated as float32(float64(a) * float64(b) + float64(c)): the product of two float32 values is exact in float64, the
sum rounds to 53 bits and then to 24 -- a double rounding that differs from the fused result only on a near-tie of the 53-bit sum.
"""
import functools

import numpy as np

from train_model import E, TINY, EXPF_ULP, gamma, ratio, silu_eval, silu_f32, f32, f64  # noqa: F401  (EXPF_ULP: the assumption silu_eval carries)

CONV_IN_ROUNDINGS = 36            # 9 taps x 4 channels, one rounding per MFMA k-step (the assumption above)


def fma32(a, b, c):
    return (f64(a) * f64(b) + f64(c)).astype(np.float32)


def _ro(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def _ht(r, *shape):
    """Heavy-tailed float32: Student t with 3 degrees of freedom."""
    return r.standard_t(3, shape).astype(np.float32)


def _plant_zeros(a):
    """A few exact zeros and -0.0 at fixed strides of the flat array."""
    flat = a.reshape(-1)
    i = np.arange(flat.size)
    flat[i % 37 == 5] = 0.0
    flat[i % 41 == 7] = -0.0
    return a


def _ub(r, N):
    """Per-image maxima that differ by a factor of at least 3 (3.7 from one image to the next, not in order)."""
    return (1.5 * 3.7 ** r.permutation(N) * r.uniform(1.0, 1.1, N)).astype(np.float32)


def _chscale(r, C):
    """Per-channel scales over 1e-2 .. 1e2 (a ratio of up to 1e4); the two extremes are always present when C >= 2."""
    s = 10.0 ** r.uniform(-2, 2, C)
    if C >= 2:
        s[0], s[C - 1] = 1e2, 1e-2
    return s.astype(np.float32)


def stage(x, ub, defect=None):
    """a = float32(x / ub[n]) as conv_in and conv_out form it (x when ub is None).  defect 'ub_prev': image n divided by ub[n - 1]."""
    x = f32(x)
    if ub is None:
        return x
    u = f32(ub)
    if defect == 'ub_prev':
        u = np.roll(u, 1)
    return x / u.reshape((-1,) + (1,) * (x.ndim - 1))


# ---------------------------------------------------------------------------------------------------------------------------
# conv_in (conv_in_kernel, yond_pack_conv_in_weight_f32)
# ---------------------------------------------------------------------------------------------------------------------------
def conv_in_model(x, ub, w, bias, slope):
    """x [N][H][W][4], ub [N] or None, w [Cout][4][3][3], bias [Cout] or None -> (out, bound) [N][H][W][Cout].

      p = sum_{tap, t} w[co][t][tap] a[y + dy - 1][x + dx - 1][t]   36 MFMA k-steps from an exact zero (the four tap-9 steps multiply a zero weight
                                   and add an exact zero): a term passes at most 36 roundings:   bp = gamma(36) S,  S = sum |w a|
      y = p + bias                 one rounding (none when bias is NULL: p + 0 is exact):         by = bp (1 + E) + E |y|
      out = y > 0 ? y : y slope    LeakyReLU with |slope| <= 1 is 1-Lipschitz, so a kernel y' on the other side of zero costs no more than
                                   by; where the kernel can be on the negative side (y - by < 0) the product rounds once:
                                                                                                  + E |slope| (|y| + by)
    slope is the float32 the entry receives.  Every line carries a few TINY for results in the subnormal range."""
    a = f64(stage(x, ub))
    N, H, W, _ = a.shape
    ap = np.pad(a, ((0, 0), (1, 1), (1, 1), (0, 0)))
    w64 = f64(f32(w)).reshape(-1, 4, 9)
    Cout = w64.shape[0]
    p = np.zeros((N, H, W, Cout))
    S = np.zeros((N, H, W, Cout))
    for tap in range(9):
        dy, dx = divmod(tap, 3)
        win = ap[:, dy:dy + H, dx:dx + W, :]
        p += win @ w64[:, :, tap].T
        S += np.abs(win) @ np.abs(w64[:, :, tap]).T
    bp = gamma(CONV_IN_ROUNDINGS) * S + np.where(S > 0, 40 * TINY, 0.0)
    if bias is None:
        y, by = p, bp
    else:
        y = p + f64(f32(bias))
        by = bp * (1 + E) + E * np.abs(y) + TINY
    s = float(np.float32(slope))
    assert abs(s) <= 1.0
    out = np.where(y > 0, y, y * s)
    bound = by + np.where(y - by < 0, E * abs(s) * (np.abs(y) + by) + (TINY if s else 0.0), 0.0)
    return out, bound


def conv_in_f32(x, ub, w, bias, slope, defect=None):
    """conv_in_kernel's steps in float32, in its order: tap pair up = 0..4, channel t = 0..3, the k = 0 half (tap 2 up) before the k = 1 half
    (tap 2 up + 1); + bias; LeakyReLU.  Defects: 'taps_dxdy' (the taps of the activation walked as (dx, dy)), 'tap9_w8' (tap 9 given tap 8's
    weight: its A operand re-reads tap 8), 'bias_group' (the bias of the neighbouring group of four channels), 'plane_off' (the PLANES4 plane
    index off by one group: what the permuted output then holds), 'ub_prev' (image n divided by ub[n - 1])."""
    a = stage(x, ub, defect)
    N, H, W, _ = a.shape
    ap = np.pad(a, ((0, 0), (1, 1), (1, 1), (0, 0)))
    w32 = f32(w).reshape(-1, 4, 9)
    Cout = w32.shape[0]
    acc = np.zeros((N, H, W, Cout), np.float32)
    for up in range(5):
        for t in range(4):
            for k in range(2):
                tap = 2 * up + k
                if tap > 8 and defect != 'tap9_w8':
                    continue                                        # a zero weight: the step adds an exact zero
                tap = min(tap, 8)
                dy, dx = divmod(tap, 3)
                if defect == 'taps_dxdy':
                    dy, dx = dx, dy
                acc = fma32(ap[:, dy:dy + H, dx:dx + W, t, None], w32[None, None, None, :, t, tap], acc)
    if bias is not None:
        b = f32(bias)
        if defect == 'bias_group':
            b = np.roll(b.reshape(-1, 4), 1, axis=0).reshape(-1)
        acc = acc + b
    out = np.where(acc > 0, acc, acc * np.float32(slope)).astype(np.float32)
    if defect == 'plane_off':
        out = np.roll(out.reshape(N, H, W, Cout // 4, 4), 1, axis=3).reshape(N, H, W, Cout)
    return out


def conv_in_pack(w):
    """yond_pack_conv_in_weight_f32's layout [Cout/32][5 tap pairs][2 halves][32 channels][4 input channels]; tap 9 is zero."""
    w = f32(w).reshape(-1, 4, 9)
    w10 = np.concatenate([w, np.zeros_like(w[:, :, :1])], axis=2)                   # [Cout][4][10]
    return np.ascontiguousarray(w10.reshape(-1, 32, 4, 5, 2).transpose(0, 3, 4, 1, 2)).reshape(-1)


def planes4_to_nhwc(p4, N, H, W, C):
    """[N][C/4][H*W][4] -> [N][H][W][C]."""
    return np.ascontiguousarray(np.asarray(p4).reshape(N, C // 4, H, W, 4).transpose(0, 2, 3, 1, 4)).reshape(N, H, W, C)


@functools.lru_cache(maxsize=None)
def conv_in_operands(N, H, W, Cout):
    """(x, ub, w, bias): signed heavy-tailed pixels with exact zeros and -0.0, output channels scaled over 1e-2 .. 1e2."""
    r = np.random.default_rng(7000 + 101 * N + 13 * H + W + Cout)
    ub = _ub(r, N)
    x = _plant_zeros(_ht(r, N, H, W, 4) * np.float32(0.3) * ub[:, None, None, None]) if H * W > 1 else _ht(r, N, H, W, 4) * ub[:, None, None, None]
    sc = _chscale(r, Cout)
    w = _ht(r, Cout, 4, 3, 3) / np.float32(6.0) * sc[:, None, None, None]
    bias = _ht(r, Cout) * sc
    return _ro(np.ascontiguousarray(x, np.float32), ub, w.astype(np.float32), bias.astype(np.float32))


CONV_IN_SHAPES = ((1, 1, 1, 32), (1, 8, 32, 32), (2, 9, 33, 64), (3, 7, 31, 32), (1, 17, 65, 96))
CONV_IN_VARIANTS = ((True, True, 0.01), (True, False, 0.2), (False, True, 0.0), (False, False, 0.01), (True, True, 0.2), (True, True, 0.0))   # (ub, bias, slope)


def conv_in_defects(shape, has_ub, has_bias):
    """The defects whose code path the case exercises."""
    N, H, W, _ = shape
    d = ['plane_off']
    if H > 1 or W > 1:
        d.append('taps_dxdy')
    if H > 1 and W > 1:
        d.append('tap9_w8')                       # tap 8 is the neighbour at (+1, +1)
    if has_bias:
        d.append('bias_group')
    if has_ub and N > 1:
        d.append('ub_prev')
    return d


# ---------------------------------------------------------------------------------------------------------------------------
# conv_out (conv_out_kernel)
# ---------------------------------------------------------------------------------------------------------------------------
def conv_out_model(feat, w, bias, x, ub):
    """feat [N][H][W][Cin], w [4][Cin], bias [4] or None, x [N][H][W][4] or None, ub [N] or None -> (out, bound) [N][H][W][4].

      d = sum_c w[o][c] feat[c]    lane part p adds its Cin / 8 products by fmaf from zero (Cin / 8 roundings), three shuffle adds join the eight
                                   parts: a term passes at most Cin / 8 + 3 roundings:           bd = gamma(Cin / 8 + 3) S,  S = sum |w feat|
      y1 = d + bias                (when bias)                                                    b1 = bd (1 + E) + E |y1|
      y2 = y1 + float32(x / ub)    (when x; the quotient only when ub; an exact operand)          b2 = b1 (1 + E) + E |y2|
      out = y2 ub                  (when ub)                                                      b3 = b2 |ub| (1 + E) + E |out|"""
    f = f64(f32(feat))
    w64 = f64(f32(w))
    Cin = w64.shape[1]
    y = f @ w64.T
    b = gamma(Cin // 8 + 3) * (np.abs(f) @ np.abs(w64).T)
    b = b + np.where(b > 0, (Cin // 8 + 3) * TINY, 0.0)
    if bias is not None:
        y = y + f64(f32(bias))
        b = b * (1 + E) + E * np.abs(y) + TINY
    if x is not None:
        y = y + f64(stage(x, ub))
        b = b * (1 + E) + E * np.abs(y) + TINY
    if ub is not None:
        u = f64(f32(ub)).reshape(-1, 1, 1, 1)
        y = y * u
        b = b * np.abs(u) * (1 + E) + E * np.abs(y) + TINY
    return y, b


def conv_out_f32(feat, w, bias, x, ub, defect=None):
    """conv_out_kernel's steps in float32.  Defects: 'no_ub_mul' (the final * ub dropped), 'res_not_div' (the residual not divided by ub),
    'drop_part' (lane part 7 left out of the reduction)."""
    feat, w32 = f32(feat), f32(w)
    N, H, W, Cin = feat.shape
    v = feat.reshape(N * H * W, Cin // 32, 8, 4)                                 # [pixel][group j][part][e]
    wr = w32.reshape(4, Cin // 32, 8, 4)                                         # [out][group j][part][e]
    o = np.zeros((N * H * W, 8, 4), np.float32)                                  # [pixel][part][out]
    for j in range(Cin // 32):
        for e in range(4):
            o = fma32(v[:, j, :, e, None], wr[:, j, :, e].T[None], o)
    if defect == 'drop_part':
        o[:, 7, :] = 0.0
    for m in (1, 2, 4):
        o = o + o[:, np.arange(8) ^ m, :]
    y = o[:, 0, :].reshape(N, H, W, 4)
    if bias is not None:
        y = y + f32(bias)
    if x is not None:
        y = y + (f32(x) if defect == 'res_not_div' else stage(x, ub))
    if ub is not None and defect != 'no_ub_mul':
        y = y * f32(ub).reshape(-1, 1, 1, 1)
    return y.astype(np.float32)


@functools.lru_cache(maxsize=None)
def conv_out_operands(N, H, W, Cin):
    """(feat, w, bias, x, ub): heavy-tailed features whose channels differ in scale by up to 1e4, the four outputs' weights by 1e2."""
    r = np.random.default_rng(7100 + 101 * N + 13 * H + W + Cin)
    ub = _ub(r, N)
    feat = _ht(r, N, H, W, Cin) * _chscale(r, Cin)
    if H * W > 1:
        _plant_zeros(feat)
    osc = np.asarray([1.0, 1e-2, 1e2, 0.3], np.float32)
    w = _ht(r, 4, Cin) / np.float32(np.sqrt(Cin)) * osc[:, None]
    bias = _ht(r, 4) * osc
    x = _ht(r, N, H, W, 4) * np.float32(0.3) * ub[:, None, None, None]
    return _ro(feat.astype(np.float32), w.astype(np.float32), bias.astype(np.float32), x.astype(np.float32), ub)


CONV_OUT_SHAPES = ((1, 1, 1, 32), (2, 5, 7, 64), (1, 3, 11, 96), (1, 1, 31, 256))
CONV_OUT_CAP_SHAPE = (1, 516, 509, 32)          # 262,644 pixels: above the grid's cap of 8192 workgroups x 32 pixels
CONV_OUT_VARIANTS = ((True, True, True), (True, False, True), (False, True, True), (False, False, True), (True, True, False))   # (x, ub, bias)


def conv_out_cases():
    return [(s, v) for s in CONV_OUT_SHAPES for v in CONV_OUT_VARIANTS] + [(CONV_OUT_CAP_SHAPE, CONV_OUT_VARIANTS[0])]


def conv_out_defects(has_x, has_ub):
    return ['drop_part'] + (['no_ub_mul'] if has_ub else []) + (['res_not_div'] if has_x and has_ub else [])


def pick(ops, flags):
    """The operands whose flag is set, None for the others."""
    return tuple(o if f else None for o, f in zip(ops, flags))


# ---------------------------------------------------------------------------------------------------------------------------
# film (film_kernel<0>, film_kernel<1>)
# ---------------------------------------------------------------------------------------------------------------------------
FILM_OUT = ('s1', 't1', 's2', 't2')


def _matvec(Wm, h, dh, bias):
    """m = Wm h + bias as a wave forms it: a lane adds its ceil(C / 64) products by fmaf from zero, six shuffle adds join the 64 lanes, the
    bias add rounds once.  A term passes at most K = ceil(C / 64) + 6 roundings; the operand h is off by dh:
        bacc = |Wm| dh + gamma(K) |Wm| (|h| + dh);   dm = bacc (1 + E) + E |m|."""
    Wm = f64(f32(Wm))
    C = Wm.shape[1]
    K = -(-C // 64) + 6
    m = h @ Wm.T + f64(f32(bias))
    op = dh @ np.abs(Wm).T
    bacc = op + gamma(K) * ((np.abs(h) + dh) @ np.abs(Wm).T) + K * TINY
    return m, bacc * (1 + E) + E * np.abs(m) + TINY


def _first(wv, bv, tv):
    """h = SiLU(fmaf(w, tv, b)): the fmaf rounds once (E |a|), silu_eval carries it through SiLU."""
    a = f64(f32(wv))[None, :] * tv[:, None] + f64(f32(bv))[None, :]
    return silu_eval(a, E * np.abs(a) + TINY)


def film_model(desc, t, ub):
    """desc: kind (0 guided, 1 SNR), C and the float32 parameters named as YondFilmDesc; t [N]; ub [N] or None -> {name: (value, bound)},
    each [N][C], in the forward kernel's order:
      tv = float32(t / ub)         exact operand (t when ub is NULL)
      h = SiLU(fmaf(w_a0, tv, b_a0));  m1 = W_a2 h + b_a2  (_matvec)                              s1 = m1, bound dm1
      guided: s = SiLU(m1 as stored: off by dm1);  m2 = W_b s + b_b;  t1 = fmaf(cb1, m1, m2):     |cb1| dm1 + dm2, one rounding E |t1|
              s2 = 1 and t2 = cb2 are exact (bound 0)
      SNR:    g = SiLU(fmaf(w_b0, tv, b_b0));  m2 = W_b g + b_b;  t1 = cb1 m1: |cb1| dm1 + E |t1|;  s2 = m2: dm2;  t2 = cb2 m2: |cb2| dm2 + E |t2|"""
    tv = f64(stage(f32(t), ub))
    h, dh = _first(desc['w_a0'], desc['b_a0'], tv)
    m1, dm1 = _matvec(desc['w_a2'], h, dh, desc['b_a2'])
    cb1, cb2 = f64(f32(desc['cb1']))[None, :], f64(f32(desc['cb2']))[None, :]
    if desc['kind'] == 0:
        s, ds = silu_eval(m1, dm1)
        m2, dm2 = _matvec(desc['w_b'], s, ds, desc['b_b'])
        t1 = cb1 * m1 + m2
        bt1 = (np.abs(cb1) * dm1 + dm2) * (1 + E) + E * np.abs(t1) + TINY
        one = np.ones_like(m1)
        return {'s1': (m1, dm1), 't1': (t1, bt1), 's2': (one, 0.0 * one), 't2': (cb2 * one, 0.0 * one)}
    g, dg = _first(desc['w_b0'], desc['b_b0'], tv)
    m2, dm2 = _matvec(desc['w_b'], g, dg, desc['b_b'])
    t1, t2 = cb1 * m1, cb2 * m2
    return {'s1': (m1, dm1), 't1': (t1, np.abs(cb1) * dm1 * (1 + E) + E * np.abs(t1) + TINY), 's2': (m2, dm2),
            't2': (t2, np.abs(cb2) * dm2 * (1 + E) + E * np.abs(t2) + TINY)}


def _matvec_f32(Wm, h, bias):
    Wm, h = f32(Wm), f32(h)
    C = Wm.shape[1]
    K = -(-C // 64)
    Wp = np.zeros((Wm.shape[0], K * 64), np.float32)
    Wp[:, :C] = Wm
    hp = np.zeros((h.shape[0], K * 64), np.float32)
    hp[:, :C] = h
    Wp, hp = Wp.reshape(-1, K, 64), hp.reshape(-1, K, 64)
    acc = np.zeros((h.shape[0], Wm.shape[0], 64), np.float32)                    # [image][row][lane]
    for k in range(K):
        acc = fma32(Wp[None, :, k, :], hp[:, None, k, :], acc)                   # (a padded column adds fmaf(0, 0, acc) = acc)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, np.arange(64) ^ o]
    return acc[:, :, 0] + f32(bias)[None, :]


def film_f32(desc, t, ub, defect=None):
    """Both stages in float32, in the kernel's order -> {name: [N][ld]}, NaN where the kernel does not write (the padding [C:ld]).
    Defects: 'clamp_row' (the clamped row's value stored: row C holds row C - 1), 'snr_t2_m1' (the SNR kind's t2 built from m1),
    't_no_ub' (t not divided by ub)."""
    C, ld = desc['C'], desc['ld']
    t32 = f32(t)
    tv = t32 if (ub is None or defect == 't_no_ub') else stage(t32, ub)
    first = lambda wv, bv: silu_f32(fma32(f32(wv)[None, :], tv[:, None], f32(bv)[None, :]))
    m1 = _matvec_f32(desc['w_a2'], first(desc['w_a0'], desc['b_a0']), desc['b_a2'])
    cb1, cb2 = f32(desc['cb1'])[None, :], f32(desc['cb2'])[None, :]
    if desc['kind'] == 0:
        m2 = _matvec_f32(desc['w_b'], silu_f32(m1), desc['b_b'])
        vals = {'s1': m1, 't1': fma32(cb1, m1, m2), 's2': np.ones_like(m1), 't2': cb2 + np.zeros_like(m1)}
    else:
        m2 = _matvec_f32(desc['w_b'], first(desc['w_b0'], desc['b_b0']), desc['b_b'])
        vals = {'s1': m1, 't1': cb1 * m1, 's2': m2, 't2': cb2 * (m1 if defect == 'snr_t2_m1' else m2)}
    out = {}
    for k, v in vals.items():
        o = np.full((t32.size, ld), np.nan, np.float32)
        o[:, :C] = v
        if defect == 'clamp_row' and C < ld:
            o[:, C] = v[:, C - 1]
        out[k] = o
    return out


def film_check(out, model, C):
    """Worst ratio over the four outputs [N][ld] against film_model's result; inf when the padding [C:ld] is not NaN any more."""
    worst = 0.0
    for k in FILM_OUT:
        o = np.asarray(out[k])
        worst = max(worst, ratio(o[:, :C], *model[k]))
        if not np.isnan(o[:, C:]).all():
            worst = float('inf')
    return worst


FILM_C = (8, 40, 264, 1024)
FILM_N = (1, 7, 8, 9)                 # below 8 images a launch has all 32 row tiles per (block, image); from 8 on, 8 tiles and a stride loop


@functools.lru_cache(maxsize=None)
def film_descs():
    """Eight descriptors (both kinds x FILM_C), ld = C rounded up to 32.  Rows of the C x C matrices (and their biases) are scaled over
    1e-2 .. 1e2; the first layers have the network's scales (sigma / ub is of the order 0.01 .. 0.3)."""
    out = []
    for kind in (0, 1):
        for C in FILM_C:
            r = np.random.default_rng(7200 + 10 * C + kind)
            d = dict(kind=kind, C=C, ld=-(-C // 32) * 32)
            sa, sb = _chscale(r, C), _chscale(r, C)[::-1].copy()
            d['w_a0'], d['b_a0'] = _ht(r, C) * 4, _ht(r, C) * np.float32(0.05)
            d['w_a2'], d['b_a2'] = _plant_zeros(_ht(r, C, C) / np.float32(C ** 0.5) * sa[:, None]), _ht(r, C) * np.float32(0.05) * sa
            d['w_b0'], d['b_b0'] = (_ht(r, C) * 4, _ht(r, C) * np.float32(0.05)) if kind else (None, None)
            d['w_b'], d['b_b'] = _ht(r, C, C) / np.float32(C ** 0.5) * sb[:, None], _ht(r, C) * np.float32(0.05) * sb
            d['cb1'], d['cb2'] = _ht(r, C) * np.float32(0.1), _ht(r, C) * np.float32(0.1)
            for k, v in d.items():
                if isinstance(v, np.ndarray):
                    d[k] = np.ascontiguousarray(v, np.float32)
                    d[k].setflags(write=False)
            out.append(d)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def film_t(N):
    """(t, ub): t = (sigma / ub) ub with sigma / ub over 0.01 .. 0.31."""
    r = np.random.default_rng(7300 + N)
    ub = _ub(r, N)
    return _ro((r.uniform(0.01, 0.31, N).astype(np.float32) * ub).astype(np.float32), ub)


def film_defects(desc, has_ub):
    return (['clamp_row'] if desc['C'] < desc['ld'] else []) + (['snr_t2_m1'] if desc['kind'] == 1 else []) + (['t_no_ub'] if has_ub else [])


# ---------------------------------------------------------------------------------------------------------------------------
# est_conv_in (est_conv_in_kernel)
# ---------------------------------------------------------------------------------------------------------------------------
def est_conv_in_model(x, w, bias):
    """x [N][H][W], w [Cout][9], bias [Cout] -> (out, bound) [N][H][W][Cout].  acc = bias, nine fmaf steps (tap t = 3 dy + dx in order): the bias
    passes nine roundings, the product of tap t the 9 - t that follow it: gamma(9) (|bias| + sum |w v|).  ReLU is 1-Lipschitz and exact."""
    x64 = f64(f32(x))
    N, H, W = x64.shape
    xp = np.pad(x64, ((0, 0), (1, 1), (1, 1)))
    w64, b64 = f64(f32(w)), f64(f32(bias))
    y = np.zeros((N, H, W, w64.shape[0])) + b64
    S = np.zeros_like(y) + np.abs(b64)
    for t in range(9):
        dy, dx = divmod(t, 3)
        win = xp[:, dy:dy + H, dx:dx + W, None]
        y += win * w64[:, t]
        S += np.abs(win) * np.abs(w64[:, t])
    return np.maximum(y, 0.0), gamma(9) * S + np.where(S > 0, 9 * TINY, 0.0)


def est_conv_in_f32(x, w, bias, defect=None):
    """The kernel's steps in float32.  Defect 'taps_dxdy': the taps walked as (dx, dy)."""
    x32, w32 = f32(x), f32(w)
    N, H, W = x32.shape
    xp = np.pad(x32, ((0, 0), (1, 1), (1, 1)))
    acc = np.zeros((N, H, W, w32.shape[0]), np.float32) + f32(bias)
    for t in range(9):
        dy, dx = divmod(t, 3)
        if defect == 'taps_dxdy':
            dy, dx = dx, dy
        acc = fma32(w32[None, None, None, :, t], xp[:, dy:dy + H, dx:dx + W, None], acc)
    return np.maximum(acc, np.float32(0.0))


@functools.lru_cache(maxsize=None)
def est_conv_in_operands(N, H, W, Cout):
    r = np.random.default_rng(7400 + 101 * N + 13 * H + W + Cout)
    x = _ht(r, N, H, W) * np.float32(0.3)
    if H * W > 1:
        _plant_zeros(x)
    sc = _chscale(r, Cout)
    return _ro(x, (_ht(r, Cout, 9) / np.float32(3.0) * sc[:, None]).astype(np.float32), (_ht(r, Cout) * np.float32(0.3) * sc).astype(np.float32))


EST_CONV_IN_SHAPES = ((1, 1, 1, 32), (2, 9, 65, 64), (1, 8, 64, 96), (1, 3, 5, 1024))


# ---------------------------------------------------------------------------------------------------------------------------
# est_head (est_head_kernel, est_head_finish_kernel)
# ---------------------------------------------------------------------------------------------------------------------------
EST_LPP, EST_PPI, EST_HEAD_BLOCKS = 16, 16, 512


def est_head_model(feat, w, bias, sq, pge):
    """feat [N][H][W][Cin], w [out_nc][Cin], bias [out_nc] -> (out, bound): the map [N][out_nc][H][W], or its spatial mean [N][out_nc] (pge).

      v = sum_c w[o][c] feat[c]    lane l adds the products of its groups l, l + 16, ... by fmaf from zero -- 4 ceil(Cin / 64) steps -- and four
                                   shuffle adds join the 16 lanes: K = 4 ceil(Cin / 64) + 4 roundings:    bv = gamma(K) S,  S = sum |w feat|
      y = v + bias                 one rounding:                                                          by = bv (1 + E) + E |y|
      y^2 (sq)                     |y'^2 - y^2| <= by (2 |y| + by), one rounding:                         by (2 |y| + by) (1 + E) + E y^2
      mean (pge)                   the float32 y summed in float64 and the quotient rounded once to float32: the mean of the per-pixel bounds
                                   plus E |mean|.  The float64 additions (at most HW of them pass a term, with the division and the
                                   conversion) add (HW + 2) 2^-53 mean |y|, kept though five orders below E."""
    f = f64(f32(feat))
    N, H, W, Cin = f.shape
    w64 = f64(f32(w))
    K = 4 * -(-Cin // 64) + 4
    y = f @ w64.T + f64(f32(bias))
    S = np.abs(f) @ np.abs(w64).T
    b = (gamma(K) * S + np.where(S > 0, K * TINY, 0.0)) * (1 + E) + E * np.abs(y) + TINY
    if sq:
        b = b * (2 * np.abs(y) + b) * (1 + E) + E * y * y + TINY
        y = y * y
    if not pge:
        return y.transpose(0, 3, 1, 2), b.transpose(0, 3, 1, 2)
    HW = H * W
    mean = y.reshape(N, HW, -1).mean(axis=1)
    mabs = np.abs(y).reshape(N, HW, -1).mean(axis=1)
    mb = b.reshape(N, HW, -1).mean(axis=1)
    return mean, mb * (1 + E) + E * np.abs(mean) + (HW + 2) * 2.0 ** -53 * (mabs + mb) + TINY


def est_head_f32(feat, w, bias, sq, pge, defect=None):
    """The kernels' steps in float32 (the mean's sums in float64).  Defects: 'sq_before_bias' (v^2 + bias), 'mean_strided' (the mean divided
    by the pixels the strided loops cover, nblk x 16 x passes, instead of HW)."""
    feat, w32 = f32(feat), f32(w)
    N, H, W, Cin = feat.shape
    nc = w32.shape[0]
    G = Cin // 4
    Kg = -(-G // EST_LPP)
    fp = np.zeros((N * H * W, Kg * EST_LPP * 4), np.float32)
    fp[:, :Cin] = feat.reshape(-1, Cin)
    wp = np.zeros((nc, Kg * EST_LPP * 4), np.float32)
    wp[:, :Cin] = w32
    fp, wp = fp.reshape(-1, Kg, EST_LPP, 4), wp.reshape(nc, Kg, EST_LPP, 4)
    v = np.zeros((N * H * W, nc, EST_LPP), np.float32)                           # [pixel][channel][lane]
    for k in range(Kg):
        for e in range(4):
            v = fma32(wp[None, :, k, :, e], fp[:, None, k, :, e], v)
    for o in (8, 4, 2, 1):
        v = v + v[:, :, np.arange(EST_LPP) ^ o]
    v = v[:, :, 0]
    b = f32(bias)[None, :]
    if sq and defect == 'sq_before_bias':
        y = v * v + b
    else:
        y = v + b
        if sq:
            y = y * y
    y = y.reshape(N, H * W, nc)
    if not pge:
        return np.ascontiguousarray(y.transpose(0, 2, 1)).reshape(N, nc, H, W)
    HW = H * W
    div = HW
    if defect == 'mean_strided':
        groups = -(-HW // EST_PPI)
        nblk = min(groups, EST_HEAD_BLOCKS)
        div = nblk * EST_PPI * -(-HW // (nblk * EST_PPI))
    return (y.astype(np.float64).sum(axis=1) / float(div)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def est_head_operands(N, H, W, Cin, out_nc):
    r = np.random.default_rng(7500 + 13 * H + W + 7 * Cin + out_nc)
    feat = _ht(r, N, H, W, Cin) * _chscale(r, Cin)
    if H * W > 1:
        _plant_zeros(feat)
    osc = np.asarray([1.0, 1e-2, 1e2, 0.3], np.float32)[:out_nc]
    w = _ht(r, out_nc, Cin) / np.float32(np.sqrt(Cin)) * osc[:, None]
    return _ro(feat.astype(np.float32), w.astype(np.float32), (_ht(r, out_nc) * osc).astype(np.float32))


EST_HEAD_N = 2
# (H, W, Cin, out_nc, sq); every case runs with both pge values.  HW = 1, 15, 17 and 8193 (above 8192 pixels per image the workgroups stride)
EST_HEAD_CASES = ((1, 1, 4, 1, 0), (1, 1, 256, 4, 1), (3, 5, 32, 2, 1), (3, 5, 60, 3, 0), (3, 5, 256, 2, 1), (1, 17, 4, 2, 0),
                  (1, 17, 60, 4, 1), (1, 17, 256, 1, 1), (3, 2731, 32, 3, 1), (3, 2731, 60, 1, 0), (3, 2731, 256, 4, 0))


def est_head_defects(sq, pge):
    return (['sq_before_bias'] if sq else []) + (['mean_strided'] if pge else [])


# ---------------------------------------------------------------------------------------------------------------------------
# exact operations
# ---------------------------------------------------------------------------------------------------------------------------
def maxpool2_model(x):
    """[N][H][W][C] -> [N][H/2][W/2][C].  (No window of the tests' data holds +0 beside -0: fmaxf may return either.)"""
    x = f32(x)
    return np.maximum(np.maximum(x[:, 0::2, 0::2], x[:, 0::2, 1::2]), np.maximum(x[:, 1::2, 0::2], x[:, 1::2, 1::2]))


def bayer2rggb_model(b):
    """[H][W] -> [H/2][W/2][4]: (R, G1, G2, B) = the 2 x 2 cell in row-major order."""
    b = f32(b)
    return np.stack([b[0::2, 0::2], b[0::2, 1::2], b[1::2, 0::2], b[1::2, 1::2]], axis=-1)


def rggb2bayer_model(p):
    p = f32(p)
    h, w, _ = p.shape
    b = np.empty((2 * h, 2 * w), np.float32)
    b[0::2, 0::2], b[0::2, 1::2], b[1::2, 0::2], b[1::2, 1::2] = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    return b


def nchw4_to_nhwc4_model(x):
    return np.ascontiguousarray(np.moveaxis(f32(x), 1, -1))


def nhwc4_to_nchw4_model(x):
    return np.ascontiguousarray(np.moveaxis(f32(x), -1, 1))


def rot90_model(x, k):
    return np.ascontiguousarray(np.rot90(f32(x), k, axes=(-2, -1)))


def image_max_model(x):
    """[N][elems] -> [N].  The entry DROPS a NaN (every step is fmaxf): the maximum of the non-NaN elements, -inf for an all-NaN image."""
    return np.fmax.reduce(f32(x), axis=1, initial=-np.inf).astype(np.float32)


MAXPOOL_SHAPES = ((1, 2, 2, 4), (2, 6, 10, 32), (1, 4, 6, 36), (3, 2, 86, 4))       # total4 = 1, 960, 54, 129: no multiple of 256
BAYER_SHAPES = ((2, 2), (6, 10), (2050, 2050))                                      # packed pixels: 1, 15, 1,050,625 (the cap is 1,048,576)
NCHW4_SHAPES = ((1, 1, 1), (3, 5, 7), (2, 725, 725))                                # 1,051,250 pixels
ROT90_CASES = tuple((s, k) for s in ((2, 10, 14), (1, 1, 9), (1, 9, 1)) for k in range(-1, 6)) + tuple(((2, 730, 720), k) for k in (1, 2, 3))
IMAGE_MAX_ELEMS = (1, 255, 4096, 4097, 1_048_576 + 1)                               # one workgroup; two; 256 workgroups and a strided tail
IMAGE_MAX_N = (1, 3)
IMAGE_MAX_KINDS = ('first', 'last', 'tail', 'neginf', 'nan')


def exact_operands(shape, seed=0, negative=False):
    """Distinct-looking finite float32 data without zeros (sign random unless negative)."""
    r = np.random.default_rng(7600 + seed + int(np.prod(shape)) % 9973)
    a = 1.0 + np.abs(_ht(r, *shape))
    s = -1.0 if negative else r.choice([-1.0, 1.0], shape)
    return np.ascontiguousarray(a * s, np.float32)


def maxpool_operands(shape, kind):
    """kind 'mixed', 'negative' (negative everywhere) or 'neginf' (-inf entries, one window all -inf)."""
    x = exact_operands(shape, 1, negative=kind != 'mixed')
    if kind == 'neginf':
        flat = x.reshape(-1)
        flat[::5] = -np.inf
        x[0, 0:2, 0:2, :] = -np.inf
    return x


@functools.lru_cache(maxsize=None)
def _image_max_base(N, elems):
    return _ro(exact_operands((N, elems), 2, negative=True))[0]


def image_max_operands(N, elems, kind):
    """All-negative data (<= -1) with the maximum -0.5 / (n + 1) planted at the first element, the last, or in the strided tail (past the 256
    workgroups' first 16 passes where there is one); 'neginf': -inf entries beside it; 'nan': NaN at the first, the last and every 97th
    element around a planted maximum in the middle, and (N > 1) image 1 all NaN."""
    x = _image_max_base(N, elems).copy()
    top = (-0.5 / (np.arange(N) + 1)).astype(np.float32)
    tail = 256 * 4096 if elems > 256 * 4096 else (3 * elems) // 4
    pos = {'first': 0, 'last': elems - 1, 'tail': tail, 'neginf': elems // 2, 'nan': elems // 2}[kind]
    if kind == 'neginf':
        x[:, ::3] = -np.inf
    if kind == 'nan':
        x[:, ::97] = np.nan
        x[:, -1] = np.nan
    x[:, pos] = top
    if kind == 'nan':
        x[:, 0] = np.nan                           # (elems == 1: the image is all NaN)
        if N > 1:
            x[1, :] = np.nan
    return x
