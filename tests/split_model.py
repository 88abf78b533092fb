"""Reference model of the split-operand arithmetic of csrc/conv_split_kernel.h, its per-output error bound, and the stress
operand generators of the split-operand tests.  Plain numpy / torch-CPU, independent of the library.

The arithmetic (header of conv_split_kernel.h): every fp32 operand a is split into h = fp16(a) and l = fp16((a - h) * 2^11);
a product a*w is h_a*h_w + 2^-11 * (h_a*l_w + l_a*h_w); fp16 x fp16 products are exact; they are summed in fp32 in 16-wide
K steps into two accumulators (h*h and the two cross terms); one FMA by 2^-11 folds the second into the first.  PARTS = 1 keeps
the h halves only.

The bound, for a float64 reference ref_i = sum_j a_j w_ij over K = taps x input channels:

    Q_i     = sqrt(sum_j (a_j w_ij)^2)
    floor_i = 2^-36 * (sum_j |w_ij| [0 < |a_j| < 2^-14] + sum_j |a_j| [0 < |w_ij| < 2^-14])       (subnormal halves)
    T_i     = (2^-22 + sqrt(K / 16) * 2^-24) * (Q_i + |ref_i|) + floor_i

2^-22 = u^2 (u = 2^-11) is the representation error of a split operand and the size of the dropped l*l term; the second term
is a random walk of K / 16 fp32 roundings.  An exact zero operand has no error and is left out of the floor.
PARTS = 1: an operand rounded to fp16 (11 significant bits) is off by up to u relative, a product by 2 u: the same formula with 4 u in place of u^2
(rel_eps() has the reasoning) and the floor of an fp16 subnormal (spacing 2^-24, so 2^-25) in place of 2^-36.

Two terms beyond the issue's formula, both derived from the instructions and not from a measurement of the kernel:
 * a kernel that applies SiLU while it stages (pre_act 1) evaluates x * rcp(1 + exp2(-x log2 e)) with v_exp_f32 and v_rcp_f32
   (1 ulp each = 2^-23) and three fp32 roundings (2^-24 each): the staged operand is off by up to 2^-23 + 2^-23 + 3 * 2^-24 <
   2^-21 relative before it is split.  Independent per operand, so it adds 2^-21 * Q_i.
 * the epilogue y = post(z * scale + shift) + res rounds each intermediate to fp32 (the library is built with
   -ffp-contract=off): 2^-24 * (|z * scale + shift| + |post| + |y|); a SiLU there adds 2^-21 * |post| as above.
The tests allow 4 * T; tests/test_split_model.py shows that the model stays below 1 * T and that single defects exceed 4 * T.
"""
import numpy as np

U = 2.0 ** -11
SUB = 2.0 ** -14                      # fp16's smallest normal number
F16_MAX = 65504.0
FACTOR = 4.0                          # the tests assert err <= FACTOR * T

DEFECTS = ('drop_lw_tap', 'drop_la_chunk', 'scale_2e-10', 'flush_subnormal_h')
DEFECTS_H = ('drop_ha_chunk', 'flush_subnormal_h')              # PARTS 1 has no l half and no 2^-11: what its bound can still catch


def split(a):
    """fp32 array -> (h, l) float16 halves as the staging / the weight packer form them."""
    a = np.asarray(a, np.float32)
    h = a.astype(np.float16)
    l = ((a - h.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return h, l


def silu_f32(x):
    """The staged SiLU as the kernels evaluate it, every step rounded to float32: x * rcp(1 + exp2(x * -log2 e)).  (numpy's exp2 and
    reciprocal are at least as accurate as v_exp_f32 / v_rcp_f32: the model has the roundings, the bound has the instructions' 1 ulp.)"""
    x = np.asarray(x, np.float32)
    with np.errstate(over='ignore'):
        e = np.exp2(x * np.float32(-1.44269504088896341)).astype(np.float32)
        return (x * (np.float32(1.0) / (np.float32(1.0) + e)).astype(np.float32)).astype(np.float32)


def model_gemm(A, Wt, parts=2, defect=None, taps=9, pre_silu=False):
    """The documented arithmetic on A [P][K] x Wt [K][Co], K ordered [tap][channel]; returns float32 [P][Co].  pre_silu: A is the raw
    tensor, the float32 SiLU is applied when it is staged (the reference is then float64 SiLU(A) @ Wt).
    defect: None or one of DEFECTS / DEFECTS_H (single faults a correct kernel does not have):
      drop_ha_chunk      the activations' h half of the first 16-channel chunk of tap 0 is zero (that chunk is not multiplied)
      drop_lw_tap        the weights' l half of tap 0 is zero
      drop_la_chunk      the activations' l half of the first 16-channel chunk of tap 0 is zero
      scale_2e-10        the epilogue folds the cross terms with 2^-10 instead of 2^-11
      flush_subnormal_h  an h half below fp16's normal range is flushed to zero (its l half is formed from the unflushed h)"""
    if pre_silu:
        A = silu_f32(A)
    ha, la = split(A)
    hw, lw = split(Wt)
    K = A.shape[1]
    assert K % 16 == 0 and K % taps == 0
    la, lw = la.copy(), lw.copy()
    sc = np.float32(2.0 ** -11)
    if defect == 'drop_lw_tap':
        lw[:K // taps] = 0
    elif defect == 'drop_la_chunk':
        la[:, :16] = 0
    elif defect == 'drop_ha_chunk':
        ha = ha.copy()
        ha[:, :16] = 0
    elif defect == 'scale_2e-10':
        sc = np.float32(2.0 ** -10)
    elif defect == 'flush_subnormal_h':
        ha = np.where(np.abs(ha.astype(np.float32)) < SUB, 0, ha).astype(np.float16)
        hw = np.where(np.abs(hw.astype(np.float32)) < SUB, 0, hw).astype(np.float16)
    elif defect is not None:
        raise ValueError(defect)
    f = lambda x: x.astype(np.float64)
    acc0 = np.zeros((A.shape[0], Wt.shape[1]), np.float32)
    acc1 = np.zeros_like(acc0)
    for k in range(0, K, 16):
        s = slice(k, k + 16)
        acc0 = (f(acc0) + f(ha[:, s]) @ f(hw[s])).astype(np.float32)
        if parts == 2:
            acc1 = (f(acc1) + f(ha[:, s]) @ f(lw[s]) + f(la[:, s]) @ f(hw[s])).astype(np.float32)
    if parts == 1:
        return acc0
    return (f(acc1) * float(sc) + f(acc0)).astype(np.float32)            # one FMA: a single rounding


def rel_eps(K, parts=2, pre_silu=False):
    """The factors of (Q + |ref|) and of Q (staged SiLU) in T.  PARTS 1: an operand rounded to fp16 is off by at most u, a
    product by 2 u in the worst case; the errors of K products are independent (a rounding error is uniform within its bounds: rms
    about 0.4 u per product), and the largest of 10^5..10^6 outputs lies near 5 sigma = 2 u Q: the coefficient is 4 u = 2^-9, which
    leaves the model a factor 2 (measured 0.44 .. 0.55 T) as the split form has (0.59 .. 0.86 T)."""
    return (U * U if parts == 2 else 4 * U) + np.sqrt(K / 16.0) * 2.0 ** -24, (2.0 ** -21 if pre_silu else 0.0)


def floor_unit(parts=2):
    return 2.0 ** -36 if parts == 2 else 2.0 ** -25


def threshold_gemm(A, Wt, ref, parts=2, pre_silu=False):
    """T [P][Co] for ref = A @ Wt in float64 (A: the operand the kernel splits -- after the pre-activation if there is one)."""
    A64, W64 = np.abs(np.asarray(A, np.float64)), np.abs(np.asarray(Wt, np.float64))
    K = A64.shape[1]
    Q = np.sqrt((A64 ** 2) @ (W64 ** 2))
    sa = ((A64 > 0) & (A64 < SUB)).astype(np.float64)
    sw = ((W64 > 0) & (W64 < SUB)).astype(np.float64)
    floor = floor_unit(parts) * (sa @ W64 + A64 @ sw)
    e, ea = rel_eps(K, parts, pre_silu)
    return e * (Q + np.abs(ref)) + ea * Q + floor


def threshold_conv(a, w, ref, stride=1, parts=2, pre_silu=False):
    """T for a convolution: a [N][C][H][W] float64 torch tensor (the operand the kernel splits: after any pre-activation),
    w [Co][C][k][k], ref = conv2d(a, w) without bias (float64)."""
    import torch
    import torch.nn.functional as F
    a, w = a.double().abs(), w.double().abs()
    k = w.shape[-1]
    conv = lambda x, y: F.conv2d(x, y, stride=stride, padding=k // 2)
    K = w.shape[1] * k * k
    Q = conv(a * a, w * w).sqrt()
    sa = ((a > 0) & (a < SUB)).double()
    sw = ((w > 0) & (w < SUB)).double()
    floor = floor_unit(parts) * (conv(sa, w) + conv(a, sw))
    e, ea = rel_eps(K, parts, pre_silu)
    return e * (Q + ref.abs()) + ea * Q + floor


def through_epilogue(Tz, z, scale=None, shift=None, post=0, slope=0.0, res=None, half_out=False):
    """Propagate T through y = post(z * scale + shift) + res (float64 torch tensors broadcastable to z; post 0 none, 1 SiLU,
    2 LeakyReLU).  Returns (y, T_y).  half_out: the value is stored as one fp16 (h-only planes): + 2^-11 |y| (half a unit
    in the 11th bit) + 2^-25 (subnormal results)."""
    import torch
    import torch.nn.functional as F
    aff = z if scale is None else z * scale
    T = Tz if scale is None else Tz * scale.abs()
    if shift is not None:
        aff = aff + shift
    if post == 1:
        p, lip, extra = F.silu(aff), 1.1, 2.0 ** -21
    elif post == 2:
        p, lip, extra = F.leaky_relu(aff, slope), max(1.0, abs(slope)), 0.0
    else:
        p, lip, extra = aff, 1.0, 0.0
    y = p if res is None else p + res
    T = lip * T + 2.0 ** -24 * (aff.abs() + p.abs() + y.abs()) + extra * p.abs()
    if half_out:
        T = T + 2.0 ** -11 * y.abs() + 2.0 ** -25
    return y, T


# ---- stress operands (seeded; everything inside the documented range |.| <= 65504) ------------------------------------------

def stress_weights(rng, Co, C, k=3, zero_out=None, fan_in=None):
    """Student-t (nu = 3) / sqrt(fan-in); every output channel scaled by 10^U(-2, 2); eight input channels x 1e3 -- in the ODD
    output channels only: where eight channels carry a thousand times the rest, Q_i is theirs and a fault in any other 16-channel
    chunk disappears below T_i (tests/test_split_model.py measures it: err / T of a lost l chunk falls to 1.3); the even output
    channels keep every chunk visible.  One global factor keeps max|w| <= 6e4.  zero_out: an output channel whose weights are zero."""
    fan_in = fan_in or C * k * k
    w = rng.standard_t(3, (Co, C, k, k)) / np.sqrt(fan_in)
    w *= 10.0 ** rng.uniform(-2, 2, (Co, 1, 1, 1))
    big = rng.choice(C, min(8, C), replace=False)
    w[1::2, big] *= 1e3
    m = np.abs(w).max()
    if m > 6.0e4:
        w *= 6.0e4 / m
    if zero_out is not None:
        w[zero_out] = 0.0
    return w.astype(np.float32)


def stress_acts(rng, shape, kind='pos', zero_ch=None):
    """rand * 10^U(-4, 0) per element ('pos'), with random signs ('signed'), or rescaled to max|a| = 6.0e4 ('big');
    shape [N][C][H][W]; zero_ch: an input channel that is exactly zero."""
    a = rng.random(shape) * 10.0 ** rng.uniform(-4, 0, shape)
    if kind == 'signed':
        a *= rng.choice([-1.0, 1.0], shape)
    elif kind == 'big':
        a *= 6.0e4 / a.max()
    elif kind == 'tame':
        a = rng.standard_normal(shape)
    elif kind != 'pos':
        raise ValueError(kind)
    if zero_ch is not None:
        a[:, zero_ch] = 0.0
    return a.astype(np.float32)


def stress_film(rng, N, C):
    """FiLM scale / shift per image and channel, magnitudes 10^U(-2, 2), random signs."""
    s = 10.0 ** rng.uniform(-2, 2, (N, C)) * rng.choice([-1.0, 1.0], (N, C))
    t = 10.0 ** rng.uniform(-2, 2, (N, C)) * rng.choice([-1.0, 1.0], (N, C))
    return s.astype(np.float32), t.astype(np.float32)


def im2col(a, k=3):
    """[C][H][W] -> [H*W][k*k*C], K ordered [tap][channel], zero padding: the GEMM a stride-1 convolution performs."""
    C, H, W = a.shape
    p = np.zeros((C, H + k - 1, W + k - 1), a.dtype)
    p[:, k // 2:k // 2 + H, k // 2:k // 2 + W] = a
    cols = [p[:, dy:dy + H, dx:dx + W].reshape(C, H * W).T for dy in range(k) for dx in range(k)]
    return np.concatenate(cols, 1)


def w2col(w):
    """[Co][C][k][k] -> [k*k*C][Co] in im2col's K order."""
    Co, C, k, _ = w.shape
    return np.ascontiguousarray(w.transpose(2, 3, 1, 0).reshape(k * k * C, Co))


def ratio_report(name, got, ref, T, ch_axis=1):
    """Print max(err / T) and the worst output channel; returns the ratio array.  got / ref / T: arrays of one shape."""
    got, ref, T = (np.asarray(x, np.float64) for x in (got, ref, T))
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / T)                 # (T = 0 and err > 0 -> inf: an exact output that is not exact)
    r = np.where(np.isfinite(got), r, np.inf)
    axes = tuple(i for i in range(r.ndim) if i != ch_axis)
    per_ch = r.max(axis=axes)
    print(f"[accuracy] {name}: max err/T={r.max():.3f} worst channel {int(per_ch.argmax())} ({per_ch.max():.3f}) "
          f"median channel {np.median(per_ch):.3f} max_abs={err.max():.3e} ref_absmax={np.abs(ref).max():.3e}")
    return r
