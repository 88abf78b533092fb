"""Float64 models, float32 simulations and per-output error bounds of the two fp32-input MFMA convolution kernels the project falls
back on -- the direct kernel conv_mfma_kernel MODE 0 (csrc/conv.hip, descriptor algo 0) and the Winograd F(2x2, 3x3) kernel
(csrc/conv_wino.hip, algo 1) -- the operand kind 'beyond fp16' that makes the range guard send a frame to them, and the restated
launch geometry of their persistent grids.  Plain torch / NumPy, independent of the library; every tensor is [N][H][W][C] float64
and the functions run on whichever device their arguments live on (tests/test_fp32_model.py checks them on the CPU against
torch's conv2d / conv_transpose2d; the GPU tests evaluate the same functions in float64 beside the kernels).

Conventions as tests/split_model.py and tests/train_model.py: a bound is a sum of absolute terms or a root-sum-square of terms, never
a multiple of the largest element; every coefficient below is derived from the instructions; the GPU tests assert err <= FACTOR * T
per element; tests/test_fp32_model.py shows that a float32 simulation of either kernel stays under 1 * T and that single defects
exceed FACTOR * T.  u = 2^-24 is the unit roundoff of float32 (round to nearest).

DIRECT KERNEL (MODE 0).  z = sum_j a_j w_j over K = taps x (C0 + C1), the operands exact float32 (no u^2 term).
  * v_mfma_f32_32x32x2_f32 performs two k-steps; tests/edge_model.py's assumption, which the measurements there confirmed, is that an
    fp32 MFMA is a chain of fused multiply-adds, ONE rounding of the accumulator per k-step: k0 = 1 product per accumulator rounding.
    K roundings of partial sums of typical size Q + |z| walk randomly:  sqrt(K / k0) u (Q + |z|),  Q = sqrt(sum_j (a_j w_j)^2).
    (Zero-padded channels add exact zeros and no rounding error: K counts the real channels.)
  * staged SiLU (silu_fast: v_exp_f32 and v_rcp_f32, 1 ulp = 2^-23 each, and three roundings): < 2^-21 relative per operand,
    independent per operand: + 2^-21 Q (split_model.silu_f32 and its term).
  * a result in the subnormal range has an absolute rounding error: + 2^-149.
EPILOGUE (epilogue_from in conv.hip, epilogue in conv_wino.hip -- the same operations): x = fmaf(z, es, et) is FUSED, one rounding:
  u |x|; LeakyReLU multiplies negative values by the slope, one rounding: u |p| (none without the activation: the factor is 1.0);
  y = p + res, one rounding: u |y| (none without a residual: the kernel adds exact zeros).  The error of z passes through multiplied by
  |es| max(1, |slope|).

WINOGRAD.  Per 2 x 2 output patch, 4 x 4 input patch d and input channel:  U_p = float32(G g G^T) (formed in float64, rounded once:
yond_pack_conv_wino_weight_f32);  V_p = B^T d B in two stages of ONE float32 subtraction or addition each (transform_store);
M_p = sum_ci U_p V_p on v_mfma_f32_16x16x4_f32 (chain of FMAs as above: Cin roundings);  y = A^T M A in two stages of two additions each.
Plane p = 4 xi + nu.  Output (a, b) of the patch reads the nine planes xi in X_a, nu in X_b, X_0 = {0, 1, 2}, X_1 = {1, 2, 3}, with
coefficients +-1.  Per plane and channel:
  * dU_p <= u |U_p|;
  * stage 1 of V: w = d_r -+ d_r', error <= u |w|; stage 2: V = w_c -+ w_c', error <= u |V| + the two stage-1 errors:
    dV_p <= u (|V_p| + a_p), a_p = the absolute sum of the FOUR inputs behind V_p (|B^T| |d| |B|).  By the zeros of B^T the nine planes of an output are
    fed by its own 3 x 3 window alone (input rows {0, 1, 2} of the tile for a = 0, {1, 2, 3} for a = 1; tests/test_fp32_model.py restates it), so nothing
    outside the window enters -- but every input enters multiplied by U_p, sums of ALL three taps of its filter row and column that cancel only
    algebraically, where the direct form keeps one product: the bound carries |U_p| (|V_p| + a_p) and grows with |input| x the largest tap of the row /
    column, D with the products themselves;
    a staged SiLU adds 2^-21 a_p;
  * the accumulation: sqrt(Cin) u (Q_p + |M_p|), Q_p = sqrt(sum_ci (U_p V_p)^2).
The roundings of different channels and planes are independent: root-sum-square over the channels and over the nine planes
    R^2 = sum_{p in 9} [ u^2 Q_p^2 + sum_ci U_p^2 (u (|V_p| + a_p) + [SiLU] 2^-21 a_p)^2 + Cin u^2 (Q_p + |M_p|)^2 ]
(a stage-1 rounding is shared by up to three planes of an output, but enters them multiplied by three different U_p).
  * the output transform, absolute: t_nu = (M_0nu + M_1nu) + M_2nu (or the differences): <= 2 u sum_xi |M_xi,nu| per t; the second stage the same
    on the t: O = 2 u (sum_{p in 9} |M_p| + sum_{nu in X_b} |t_nu|).
    T_z = R + O + 2^-149, then the epilogue as above (this kernel fuses the FiLM multiply-add too).
The direct-form bound D of the same output (K = 9 Cin) is returned beside it; T / D measures how much wider the Winograd fallback is.
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import split_model as S

FACTOR = S.FACTOR                     # the tests assert err <= FACTOR * T
U32 = 2.0 ** -24
K0 = 1                                # products per accumulator rounding of the fp32 MFMAs (docstring)
SILU_REL = 2.0 ** -21
TINY = 2.0 ** -149
KINDS = ('tame', 'pos', 'signed', 'big', 'beyond')

BT = ((1, 0, -1, 0), (0, 1, 1, 0), (0, -1, 1, 0), (0, 1, 0, -1))
GM = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))
AT = ((1, 1, 1, 0), (0, 1, -1, -1))


# ---- operands ---------------------------------------------------------------------------------------------------------------------

def stress_acts(rng, shape, kind):
    """split_model.stress_acts ([N][C][H][W] float32) with one more kind, 'beyond': the signed set with about 1e-3 of the elements replaced
    by values of magnitude 6.6e4 .. 1e6 (log-uniform, both signs) -- isolated, so each has ordinary neighbours.  One such value trips the range guard."""
    if kind != 'beyond':
        return S.stress_acts(rng, shape, kind)
    a = S.stress_acts(rng, shape, 'signed').astype(np.float64)
    hit = rng.random(shape) < 1e-3
    big = 10.0 ** rng.uniform(np.log10(6.6e4), 6.0, shape) * rng.choice([-1.0, 1.0], shape)
    return np.where(hit, big, a).astype(np.float32)


def stress_weights(rng, Co, C, k, kind, fan_in=None):
    """'tame': normal / sqrt(fan-in); 'beyond': split_model.stress_weights rescaled to max |w| = 2e5 (a weight above 65504 keeps a layer on these
    kernels); every other kind: split_model.stress_weights."""
    fan_in = fan_in or C * k * k
    if kind == 'tame':
        return (rng.standard_normal((Co, C, k, k)) / np.sqrt(fan_in)).astype(np.float32)
    w = S.stress_weights(rng, Co, C, k, fan_in=fan_in)
    if kind == 'beyond':
        w = (w.astype(np.float64) * (2.0e5 / np.abs(w).max())).astype(np.float32)
    return w


def stress_film(rng, N, C, kind):
    """split_model.stress_film; 'tame': normal draws; 'beyond': every sixteenth channel's scale and shift x 1e3 (up to 1e5)."""
    if kind == 'tame':
        return rng.standard_normal((N, C)).astype(np.float32), rng.standard_normal((N, C)).astype(np.float32)
    s, t = S.stress_film(rng, N, C)
    if kind == 'beyond':
        s[:, ::16] *= 1e3
        t[:, ::16] *= 1e3
    return s, t


# ---- float64 models ---------------------------------------------------------------------------------------------------------------

def silu64(x):
    return x * torch.sigmoid(x)


def pad1(x, k):
    p = k // 2
    return F.pad(x, (0, 0, p, p, p, p)) if p else x


def conv_nhwc(x, w, ksize=3, stride=1, padded=False):
    """x [N][H][W][C], w [Co][C][k][k] -> [N][Ho][Wo][Co], zero padding k // 2, as a sum of k * k matrix products (padded: x carries its border)."""
    xp = x if padded else pad1(x, ksize)
    H, W = xp.shape[1] - 2 * (ksize // 2), xp.shape[2] - 2 * (ksize // 2)
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    out = None
    for dy in range(ksize):
        for dx in range(ksize):
            s = xp[:, dy:dy + (Ho - 1) * stride + 1:stride, dx:dx + (Wo - 1) * stride + 1:stride, :]
            o = s @ w[:, :, dy, dx].t()
            out = o if out is None else out + o
    return out


def convt_nhwc(x, w):
    """ConvTranspose2d 2 x 2 stride 2: x [N][H][W][Ci], w [Ci][Co][2][2] -> [N][2H][2W][Co]."""
    N, H, W, _ = x.shape
    Co = w.shape[1]
    o = torch.stack([torch.stack([x @ w[:, :, dy, dx] for dx in range(2)], 3) for dy in range(2)], 2)     # [N][H][2][W][2][Co]
    return o.reshape(N, 2 * H, 2 * W, Co)


def linear_op(x, w, ksize, stride, shuffle, padded=False):
    return convt_nhwc(x, w) if shuffle else conv_nhwc(x, w, ksize, stride, padded)


def film_vec(v, N):
    """[N or 1][C] (or None) -> broadcastable to [N][H][W][C]."""
    return None if v is None else v[:, None, None, :]


def epilogue(Tz, z, es=None, et=None, slope=None, res=None):
    """y = LeakyReLU(fmaf(z, es, et)) + res and its bound (docstring: EPILOGUE).  es / et [N or 1][C]; slope None: no activation."""
    es, et = film_vec(es, z.shape[0]), film_vec(et, z.shape[0])
    x = z if es is None else z * es
    T = Tz if es is None else Tz * es.abs()
    if et is not None:
        x = x + et
    T = T + U32 * x.abs()
    p = x
    if slope is not None:
        p = torch.where(x > 0, x, x * slope)
        T = T * max(1.0, abs(slope)) + U32 * p.abs()
    y = p
    if res is not None:
        y = p + res
        T = T + U32 * y.abs()
    return y, T


def direct_bound(a, w, z, ksize, stride, shuffle, pre):
    """T_z of the direct kernel for z = linear_op(a, w): a the staged operand in float64 (after any SiLU)."""
    K = w.shape[0 if shuffle else 1] * (1 if shuffle else ksize * ksize)
    Q = linear_op(a * a, w * w, ksize, stride, shuffle).sqrt()
    return np.sqrt(K / K0) * U32 * (Q + z.abs()) + (SILU_REL * Q if pre else 0.0) + TINY, Q


def _q_out(Q, es):
    return Q if es is None else Q * film_vec(es, Q.shape[0]).abs()


def direct_model(x, w, ksize=3, stride=1, shuffle=False, pre=False, es=None, et=None, slope=None, res=None):
    """Float64 reference of one layer of the direct kernel and its per-output bound: dict(y, T, Q) (Q scaled by |es|: the output's condition)."""
    a = silu64(x) if pre else x
    z = linear_op(a, w, ksize, stride, shuffle)
    Tz, Q = direct_bound(a, w, z, ksize, stride, shuffle, pre)
    y, T = epilogue(Tz, z, es, et, slope, res)
    return dict(y=y, T=T, Q=_q_out(Q, es), D=None)


# ---- Winograd -----------------------------------------------------------------------------------------------------------------------

def wino_U(w, round32=True):
    """[Co][Ci][3][3] -> U [16][Co][Ci]: G g G^T in float64, rounded once to float32 (round32)."""
    G = torch.tensor(GM, dtype=torch.float64, device=w.device)
    U = torch.einsum('xa,oiab,nb->xnoi', G, w.double(), G).reshape(16, w.shape[0], w.shape[1])
    return U.float().double() if round32 else U


def wino_patches(a):
    """[N][H][W][C] -> d [4][4][N][PH][PW][C]: the 4 x 4 input patch (rows 2i - 1 .. 2i + 2) of every 2 x 2 output patch, zero outside the image."""
    N, H, W, C = a.shape
    PH, PW = (H + 1) // 2, (W + 1) // 2
    ap = F.pad(a, (0, 0, 1, 2 * PW - W + 1, 1, 2 * PH - H + 1))
    return torch.stack([torch.stack([ap[:, r:r + 2 * PH:2, c:c + 2 * PW:2, :] for c in range(4)], 0) for r in range(4)], 0)


def _r32(t):
    return t.float().double()


def wino_V(d, round32, bt=BT):
    """B^T d B in the kernel's two stages (rows, then columns), each one addition or subtraction; round32: every result rounded to float32.
    Returns V [16][N][PH][PW][C]."""
    r = _r32 if round32 else (lambda t: t)
    w = [[None] * 4 for _ in range(4)]
    for xi in range(4):
        for c in range(4):
            s = None
            for rr in range(4):
                if bt[xi][rr]:
                    s = bt[xi][rr] * d[rr][c] if s is None else s + bt[xi][rr] * d[rr][c]
            w[xi][c] = r(s)
    V = []
    for xi in range(4):
        for nu in range(4):
            s = None
            for c in range(4):
                if BT[nu][c]:
                    s = BT[nu][c] * w[xi][c] if s is None else s + BT[nu][c] * w[xi][c]
            V.append(r(s))
    return torch.stack(V, 0)


def wino_out(M, round32):
    """A^T M A in the kernel's two stages of two additions each: M [16][...] -> y [2][2][...]."""
    r = _r32 if round32 else (lambda t: t)
    t0 = [r(r(M[0 + nu] + M[4 + nu]) + M[8 + nu]) for nu in range(4)]
    t1 = [r(r(M[4 + nu] - M[8 + nu]) - M[12 + nu]) for nu in range(4)]
    y = []
    for t in (t0, t1):
        y.append([r(r(t[0] + t[1]) + t[2]), r(r(t[1] - t[2]) - t[3])])
    return y


def wino_unpatch(y, H, W):
    """y [2][2] of [N][PH][PW][Co] -> [N][H][W][Co]."""
    N, PH, PW, Co = y[0][0].shape
    o = torch.stack([torch.stack([y[a][b] for b in range(2)], 3) for a in range(2)], 2)        # [N][PH][2][PW][2][Co]
    return o.reshape(N, 2 * PH, 2 * PW, Co)[:, :H, :W, :]


WINO_CH_ORDER = (0, 2, 4, 6, 1, 3, 5, 7)      # channels of an 8-channel chunk in the order the two MFMAs of a 16 x 16 block fold them (lane group kq, kk)


def wino_forward(a, w, round32=False, bt=BT, drop_plane=None):
    """The Winograd arithmetic on the staged operand a [N][H][W][C]: round32 False -- exact algebra in float64 (equals the direct convolution);
    True -- the kernel's float32 arithmetic (U rounded once, V in two rounded stages, an FMA chain per plane in the kernel's channel order, the
    output transform in four rounded additions).  bt / drop_plane: defects."""
    N, H, W, C = a.shape
    U = wino_U(w, round32)
    V = wino_V(wino_patches(a), round32, bt)
    if round32:
        M = torch.zeros((16,) + V.shape[1:4] + (w.shape[0],), dtype=torch.float64, device=a.device)
        for c0 in range(0, C, 8):
            for j in WINO_CH_ORDER:
                ci = c0 + j
                M = _r32(M + V[..., ci:ci + 1] * U[:, None, None, None, :, ci])
    else:
        M = torch.einsum('pnhwc,poc->pnhwo', V, U)
    if drop_plane is not None:
        M[drop_plane] = 0.0
    return wino_unpatch(wino_out(M, round32), H, W)


def wino_bound(a, w, pre):
    """(T_z, M-domain reference z) of the Winograd kernel for the staged operand a (docstring: WINOGRAD), plane by plane."""
    N, H, W, C = a.shape
    Co = w.shape[0]
    U = wino_U(w, True)
    d = wino_patches(a)
    V = wino_V(d, False)
    absBT = [[abs(v) for v in row] for row in BT]
    dabs = d.abs()
    R2 = [[0.0, 0.0], [0.0, 0.0]]
    O1 = [[0.0, 0.0], [0.0, 0.0]]
    tabs = [[None] * 4 for _ in range(2)]
    X = ((0, 1, 2), (1, 2, 3))
    Ms = []
    for p in range(16):
        xi, nu = p >> 2, p & 3
        ap = sum(absBT[xi][r] * absBT[nu][c] * dabs[r][c] for r in range(4) for c in range(4) if absBT[xi][r] * absBT[nu][c])
        Up, Vp = U[p], V[p]
        Mp = Vp @ Up.t()
        Qp2 = (Vp * Vp) @ (Up * Up).t()
        dV = U32 * (Vp.abs() + ap) + (SILU_REL * ap if pre else 0.0)
        Z = U32 ** 2 * Qp2 + (dV * dV) @ (Up * Up).t() + C * U32 ** 2 * (Qp2.sqrt() + Mp.abs()) ** 2
        Ms.append(Mp)
        for ia in range(2):
            for ib in range(2):
                if xi in X[ia] and nu in X[ib]:
                    R2[ia][ib] = R2[ia][ib] + Z
                    O1[ia][ib] = O1[ia][ib] + Mp.abs()
    for ia in range(2):
        for nu in range(4):
            tabs[ia][nu] = sum(AT[ia][xi] * Ms[4 * xi + nu] for xi in range(4) if AT[ia][xi]).abs()
    T = [[None, None], [None, None]]
    for ia in range(2):
        for ib in range(2):
            O = 2.0 * U32 * (O1[ia][ib] + sum(tabs[ia][nu] for nu in X[ib]))
            T[ia][ib] = R2[ia][ib].sqrt() + O + TINY
    return wino_unpatch(T, H, W)


def wino_model(x, w, pre=False, es=None, et=None, slope=None, res=None):
    """Float64 reference (the DIRECT convolution) of one layer of the Winograd kernel, its per-output bound T, and the direct-form bound D of the
    same output: dict(y, T, D, Q)."""
    a = silu64(x) if pre else x
    z = conv_nhwc(a, w, 3, 1)
    Tz = wino_bound(a, w, pre)
    Dz, Q = direct_bound(a, w, z, 3, 1, False, pre)
    y, T = epilogue(Tz, z, es, et, slope, res)
    _, D = epilogue(Dz, z, es, et, slope, res)
    return dict(y=y, T=T, D=D, Q=_q_out(Q, es))


# ---- float32 simulations of the kernels' arithmetic ---------------------------------------------------------------------------------------

def silu_f32(x):
    """split_model.silu_f32 on a float64 tensor holding float32 values."""
    return torch.from_numpy(S.silu_f32(x.cpu().numpy().astype(np.float32)).astype(np.float64)).to(x.device)


def epilogue_f32(z, es=None, et=None, slope=None, res=None):
    es, et = film_vec(es, z.shape[0]), film_vec(et, z.shape[0])
    x = z if es is None else z * es
    if et is not None:
        x = x + et
    x = _r32(x)                                                 # fmaf: one rounding
    if slope is not None:
        x = torch.where(x > 0, x, _r32(x * slope))
    return x if res is None else _r32(x + res)


def sim_direct(x, w, ksize=3, stride=1, shuffle=False, kc=16, pre=False, es=None, et=None, slope=None, res=None):
    """conv_mfma_kernel MODE 0 in float32: (chunk of kc channels) x (tap) x (group of 8) x (k-step t) x (half h) with channel q*8 + h*4 + t, one FMA
    (one rounding) per product.  shuffle: the four sub-position GEMMs of the transposed layer, each a 1 x 1 walk."""
    a = silu_f32(x) if pre else x
    if shuffle:
        wl = [w[:, :, dy, dx].t().contiguous()[:, :, None, None] for dy in range(2) for dx in range(2)]
        zs = [_sim_direct_z(a, wi, 1, 1, kc) for wi in wl]
        N, H, W, _ = x.shape
        z = torch.stack([torch.stack([zs[2 * dy + dx] for dx in range(2)], 3) for dy in range(2)], 2).reshape(N, 2 * H, 2 * W, -1)
    else:
        z = _sim_direct_z(a, w, ksize, stride, kc)
    return epilogue_f32(z, es, et, slope, res)


def _sim_direct_z(a, w, ksize, stride, kc):
    xp = pad1(a, ksize)
    N, H, W, C = a.shape
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    acc = torch.zeros(N, Ho, Wo, w.shape[0], dtype=torch.float64, device=a.device)
    for c0 in range(0, C, kc):
        for dy in range(ksize):
            for dx in range(ksize):
                s = xp[:, dy:dy + (Ho - 1) * stride + 1:stride, dx:dx + (Wo - 1) * stride + 1:stride, :]
                for q in range(kc // 8):
                    for t in range(4):
                        for h in range(2):
                            ci = c0 + q * 8 + h * 4 + t
                            acc = _r32(acc + s[..., ci:ci + 1] * w[:, ci, dy, dx])
    return acc


def sim_wino(x, w, pre=False, es=None, et=None, slope=None, res=None, **defect):
    a = silu_f32(x) if pre else x
    return epilogue_f32(wino_forward(a, w, True, **defect), es, et, slope, res)


# ---- launch geometry, restated from the kernels' constants ---------------------------------------------------------------------------------
# form -> (tile rows, tile columns, channel-tile width, channel chunk, persistent slots = 256 CUs x workgroups per CU, deferred epilogue)
FORMS = {
    'wino64': dict(th=8, tw=32, tn=64, kc=8, slots=256, defer=False),           # conv_wino_kernel<64, 8, 8, 2>: one workgroup per CU
    'wino32': dict(th=16, tw=32, tn=32, kc=8, slots=256, defer=False),          # conv_wino_kernel<32, 16, 8, 1>
    's2_32': dict(th=4, tw=32, tn=32, kc=8, slots=512, defer=False),            # conv_mfma_kernel<3, 2, 4, 32, 8>: two workgroups per CU
    'k1_64': dict(th=8, tw=32, tn=64, kc=16, slots=512, defer=False),           # <1, 1, 8, 64, 16>: two
    'k1_32': dict(th=8, tw=32, tn=32, kc=16, slots=768, defer=False),           # <1, 1, 8, 32, 16>: three
    's1_32_16': dict(th=8, tw=32, tn=32, kc=16, slots=256, defer=True),         # <3, 1, 8, 32, 16>: one workgroup per CU, deferred epilogue
    's1_64_16': dict(th=8, tw=32, tn=64, kc=16, slots=256, defer=True),
    's1_32_8': dict(th=8, tw=32, tn=32, kc=8, slots=512, defer=False),          # <3, 1, 8, 32, 8>: two
    's1_64_8': dict(th=8, tw=32, tn=64, kc=8, slots=512, defer=False),
    's2_64': dict(th=8, tw=32, tn=64, kc=8, slots=256, defer=True),             # <3, 2, 8, 64, 8>: one, deferred
}


def geometry(form, gemm_n, cin, N, Ho, Wo):
    """Tile count, grid, chunks per tile and the walk of a launch: dict(tiles, grid, chunks, rounds, nct, ntx, nty, remap)."""
    f = FORMS[form]
    nct = gemm_n // f['tn']
    ntx, nty = (Wo + f['tw'] - 1) // f['tw'], (Ho + f['th'] - 1) // f['th']
    tiles = nct * ntx * nty * N
    grid = min(tiles, f['slots'])
    chunks = cin // f['kc']
    return dict(f, tiles=tiles, grid=grid, chunks=chunks, rounds=(tiles + grid - 1) // grid, nct=nct, ntx=ntx, nty=nty, remap=grid % 8 == 0,
                defer=f['defer'] and chunks >= 2)


def decode(t, g):
    """Logical tile t -> (image, channel tile, first output row, first output column), as both kernels decode it."""
    tpi = g['nct'] * g['ntx'] * g['nty']
    n, b = divmod(t, tpi)
    ct = b % g['nct']
    b //= g['nct']
    return n, ct, (b // g['ntx']) * g['th'], (b % g['ntx']) * g['tw']


# ---- the walk cases of the GPU tests (tests/test_hip_fp32_mfma.py); tests/test_fp32_model.py pins the regime each one claims ---------------------
REGIMES = ('lt_slots_not8', 'eq_slots', 'one_to_two', 'gt_two', 'chunks1', 'chunks2', 'chunks3', 'chunks4+', 'ct2_img2', 'ragged', '1x1', '1row', 'two_src')
MANDATORY = ('wino64', 'wino32', 's2_32', 'k1_64', 'k1_32')
# what a form cannot reach: the direct kernels take C0 + C1 in multiples of 16 (yond_conv_config), so 8-channel chunks come in pairs
UNREACHABLE = {'s2_32': ('chunks1', 'chunks3')}


def case(name, form, splits, cout, N, H, W, claims, ks=3, st=1, sh=False, pre=False, film=None, slope=None, res=False, force=None):
    """splits: input channels per source; H, W: INPUT size (GEMM-M extent of a transposed layer); film: None = bias, 'batch' = per-image scale / shift
    (ebatch 1); force: (tn, kc) put into the descriptor by hand where yond_conv_config does not choose that form at this extent."""
    return dict(name=name, form=form, splits=tuple(splits), cout=cout, N=N, H=H, W=W, claims=tuple(claims), ks=ks, st=st, sh=sh, pre=pre, film=film,
                slope=slope, res=res, force=force)


FR = dict(film='batch', slope=0.2, res=True)          # consecutive tiles differ in scale / shift vector and residual
CASES = [
    # conv_wino_kernel<64, 8, 8, 2>: 8 x 32 tiles, 256 slots, 8-channel chunks
    case('w64_1x1', 'wino64', (8,), 64, 1, 1, 1, ('1x1', 'chunks1', 'lt_slots_not8')),
    case('w64_row', 'wino64', (16,), 64, 3, 1, 70, ('1row', 'chunks2', 'lt_slots_not8', 'ragged')),
    case('w64_eq', 'wino64', (24,), 128, 2, 64, 256, ('eq_slots', 'chunks3'), **FR),
    case('w64_mid', 'wino64', (8, 16), 128, 2, 52, 400, ('one_to_two', 'chunks3', 'two_src', 'ragged', 'ct2_img2'), **FR),
    case('w64_far', 'wino64', (16,), 128, 3, 56, 416, ('gt_two', 'chunks2', 'ct2_img2'), **FR),
    case('w64_deep', 'wino64', (32,), 128, 2, 52, 400, ('one_to_two', 'chunks4+', 'ragged'), pre=True),
    case('w64_step', 'wino64', (8,), 128, 3, 56, 416, ('gt_two', 'chunks1', 'ct2_img2'), **FR),
    # conv_wino_kernel<32, 16, 8, 1>: 16 x 32 tiles, 256 slots, one V image
    case('w32_1x1', 'wino32', (8,), 32, 1, 1, 1, ('1x1', 'chunks1', 'lt_slots_not8')),
    case('w32_row', 'wino32', (16,), 32, 3, 1, 70, ('1row', 'chunks2', 'lt_slots_not8', 'ragged')),
    case('w32_eq', 'wino32', (24,), 32, 4, 128, 256, ('eq_slots', 'chunks3'), **FR),
    case('w32_mid', 'wino32', (8, 16), 96, 2, 100, 272, ('one_to_two', 'chunks3', 'two_src', 'ragged', 'ct2_img2'), **FR),
    case('w32_far', 'wino32', (16,), 96, 3, 100, 272, ('gt_two', 'chunks2', 'ct2_img2'), **FR),
    case('w32_deep', 'wino32', (32,), 96, 2, 100, 272, ('one_to_two', 'chunks4+', 'ragged'), pre=True),
    case('w32_step', 'wino32', (8,), 96, 3, 100, 272, ('gt_two', 'chunks1', 'ct2_img2'), **FR),
    # conv_mfma_kernel<3, 2, 4, 32, 8>: 4 x 32 output tiles, 512 slots; odd H and W
    case('s2_1x1', 's2_32', (16,), 32, 1, 1, 1, ('1x1', 'chunks2', 'lt_slots_not8'), st=2),
    case('s2_row', 's2_32', (16,), 32, 3, 1, 131, ('1row', 'chunks2', 'lt_slots_not8', 'ragged', 'odd_s2'), st=2),
    case('s2_eq', 's2_32', (16,), 64, 2, 63, 1023, ('eq_slots', 'chunks2', 'odd_s2'), st=2, **FR),
    case('s2_mid', 's2_32', (16, 32), 64, 3, 59, 999, ('one_to_two', 'chunks4+', 'two_src', 'ragged', 'odd_s2', 'ct2_img2'), st=2, **FR),
    case('s2_far', 's2_32', (16,), 128, 3, 59, 999, ('gt_two', 'chunks2', 'ragged', 'odd_s2', 'ct2_img2'), st=2, **FR),
    # conv_mfma_kernel<1, 1, 8, 64, 16>: 512 slots; 1 x 1 two-source and the transposed form
    case('k64_1x1', 'k1_64', (16,), 64, 1, 1, 1, ('1x1', 'chunks1', 'lt_slots_not8'), ks=1),
    case('k64_row', 'k1_64', (32,), 64, 3, 1, 70, ('1row', 'chunks2', 'lt_slots_not8', 'ragged'), ks=1, sh=True),
    case('k64_eq', 'k1_64', (16, 32), 128, 4, 64, 256, ('eq_slots', 'chunks3', 'two_src'), ks=1, **FR),
    case('k64_mid', 'k1_64', (32,), 64, 5, 26, 200, ('one_to_two', 'chunks2', 'ragged', 'ct2_img2'), ks=1, sh=True, **FR),
    case('k64_far', 'k1_64', (16, 48), 256, 3, 52, 400, ('gt_two', 'chunks4+', 'two_src', 'ragged', 'ct2_img2'), ks=1, **FR),
    case('k64_step', 'k1_64', (16,), 64, 5, 26, 200, ('one_to_two', 'chunks1', 'ragged', 'ct2_img2'), ks=1, sh=True, **FR),
    # conv_mfma_kernel<1, 1, 8, 32, 16>: 768 slots
    case('k32_1x1', 'k1_32', (16,), 32, 1, 1, 1, ('1x1', 'chunks1', 'lt_slots_not8'), ks=1),
    case('k32_row', 'k1_32', (32,), 32, 3, 1, 70, ('1row', 'chunks2', 'lt_slots_not8', 'ragged'), ks=1, sh=True),
    case('k32_eq', 'k1_32', (16, 32), 96, 4, 64, 256, ('eq_slots', 'chunks3', 'two_src'), ks=1, **FR),
    case('k32_mid', 'k1_32', (32,), 32, 8, 26, 200, ('one_to_two', 'chunks2', 'ragged', 'ct2_img2'), ks=1, sh=True, **FR),
    case('k32_far', 'k1_32', (16, 48), 96, 6, 52, 400, ('gt_two', 'chunks4+', 'two_src', 'ragged', 'ct2_img2'), ks=1, **FR),
    case('k32_step', 'k1_32', (16,), 32, 8, 26, 200, ('one_to_two', 'chunks1', 'ragged', 'ct2_img2'), ks=1, sh=True, **FR),
    # the other forms: between G and 2 G tiles with a residual and per-image FiLM.  16-channel chunks on one workgroup per CU (deferred epilogue) are
    # what yond_conv_config returns for an unknown extent; with the extent it prefers the 8-channel form at every tile count in (256, 512): forced
    case('s1_32_16', 's1_32_16', (32,), 96, 2, 52, 200, ('one_to_two', 'chunks2', 'ragged', 'ct2_img2'), pre=True, force=(32, 16), **FR),
    case('s1_64_16', 's1_64_16', (32,), 128, 3, 52, 200, ('one_to_two', 'chunks2', 'ragged', 'ct2_img2'), pre=True, force=(64, 16), **FR),
    case('s1_32_8', 's1_32_8', (32,), 96, 3, 100, 200, ('one_to_two', 'chunks4+', 'ragged', 'ct2_img2'), pre=True, **FR),
    case('s1_64_8', 's1_64_8', (32,), 192, 3, 116, 200, ('one_to_two', 'chunks4+', 'ragged', 'ct2_img2'), pre=True, **FR),
    # <3, 2, 8, 64, 8>: the library never picks it for a stride-2 layer; descriptor filled by hand from yond_pack_conv_weight_f32(tn 64, kc 8)
    case('s2_64', 's2_64', (16,), 128, 3, 103, 399, ('one_to_two', 'chunks2', 'ragged', 'odd_s2', 'ct2_img2'), st=2, force=(64, 8), **FR),
]


def case_geometry(c):
    Ho, Wo = ((c['H'] + 1) // 2, (c['W'] + 1) // 2) if c['st'] == 2 else (c['H'], c['W'])
    gemm_n = 4 * c['cout'] if c['sh'] else c['cout']
    return geometry(c['form'], gemm_n, sum(c['splits']), c['N'], Ho, Wo), gemm_n, Ho, Wo


def claim_holds(claim, c):
    """The regime `claim` restated as a predicate of the case's geometry."""
    g, gemm_n, Ho, Wo = case_geometry(c)
    t, s = g['tiles'], g['slots']
    if claim == 'lt_slots_not8':
        return t < s and t % 8 != 0 and not g['remap']
    if claim == 'eq_slots':
        return t == s
    if claim == 'one_to_two':
        return s < t < 2 * s
    if claim == 'gt_two':
        return t > 2 * s and g['rounds'] >= 3
    if claim.startswith('chunks'):
        return g['chunks'] >= 4 if claim == 'chunks4+' else g['chunks'] == int(claim[6:])
    if claim == 'ct2_img2':
        return g['nct'] >= 2 and c['N'] >= 2 and t > s and c['film'] == 'batch' and c['res']
    if claim == 'ragged':
        return Wo % g['tw'] != 0 and (Ho % g['th'] != 0 or Ho == 1)
    if claim == '1x1':
        return c['H'] == 1 and c['W'] == 1
    if claim == '1row':
        return c['H'] == 1 and c['W'] > 1
    if claim == 'odd_s2':
        return c['st'] == 2 and c['H'] % 2 == 1 and c['W'] % 2 == 1
    if claim == 'two_src':
        return len(c['splits']) == 2 and c['splits'][0] != c['splits'][1] and (not c['form'].startswith('wino') or c['splits'][0] == 8)
    raise ValueError(claim)


def case_operands(c, kind, device='cpu'):
    """Seeded operands of a case as float64 [N][H][W][C] tensors holding float32 values: dict(xs, w (OIHW; transposed: [Ci][Co][2][2]), bias, es, et, res)."""
    rng = np.random.default_rng([7, zlib.crc32(c['name'].encode()), KINDS.index(kind)])
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double().to(device)
    N, H, W, Co, cin = c['N'], c['H'], c['W'], c['cout'], sum(c['splits'])
    xs = [T(stress_acts(rng, (N, s, H, W), kind).transpose(0, 2, 3, 1)) for s in c['splits']]
    k = 2 if c['sh'] else c['ks']
    w = stress_weights(rng, Co, cin, k, kind, fan_in=cin * (1 if c['sh'] else k * k))
    if c['sh']:
        w = w.transpose(1, 0, 2, 3)
    o = dict(xs=xs, w=T(w), bias=None, es=None, et=None, res=None)
    if c['film'] == 'batch':
        es, et = stress_film(rng, N, Co, kind)
        o['es'], o['et'] = T(es), T(et)
    else:
        o['bias'] = T((10.0 ** rng.uniform(-2, 2, Co) * rng.choice([-1.0, 1.0], Co)).astype(np.float32))
    if c['res']:
        g, gemm_n, Ho, Wo = case_geometry(c)
        f = 2 if c['sh'] else 1
        o['res'] = T(stress_acts(rng, (N, Co, f * Ho, f * Wo), 'signed' if kind in ('big', 'beyond') else kind).transpose(0, 2, 3, 1))
    return o


def case_et(o):
    return o['et'] if o['et'] is not None else o['bias'][None, :]


def case_model(c, o):
    """dict(y, T, D, Q) of a case on its operands: the Winograd model for the Winograd forms, else the direct model."""
    x = torch.cat(o['xs'], 3)
    if c['form'].startswith('wino'):
        return wino_model(x, o['w'], c['pre'], o['es'], case_et(o), c['slope'], o['res'])
    return direct_model(x, o['w'], c['ks'], c['st'], c['sh'], c['pre'], o['es'], case_et(o), c['slope'], o['res'])


def case_sim(c, o):
    """The float32 simulation of the case's kernel on its operands."""
    x = torch.cat(o['xs'], 3)
    kw = dict(pre=c['pre'], es=o['es'], et=case_et(o), slope=c['slope'], res=o['res'])
    if c['form'].startswith('wino'):
        return sim_wino(x, o['w'], **kw)
    return sim_direct(x, o['w'], c['ks'], c['st'], c['sh'], FORMS[c['form']]['kc'], **kw)


def ill_conditioned(m):
    """Fraction of the outputs with T > 0.1 |ref| + 0.1 Q: above 1 % a case says nothing."""
    return float((m['T'] > 0.1 * m['y'].abs() + 0.1 * m['Q']).double().mean())


def expected_tag(c):
    """The plan.prof tag engine._conv gives the case's launch."""
    f = FORMS[c['form']]
    return f"conv_wino_kernel<{f['tn']}>" if c['form'].startswith('wino') else f"conv_mfma_kernel<{c['ks']},{c['st']},8,{f['tn']},{f['kc']}>"


# ---- single defects a correct kernel does not have, in float64 on top of the reference (their error is far above any rounding) ---------------------
DEFECTS = ('prev_ct_weights', 'prev_image_film', 'next_tile_residual', 'acc_not_cleared', 'src1_from_src0', 'oob_row_pixel0', 'silu_border_only')
DEFECTS_WINO = ('bt_sign_row', 'drop_plane')


def defective(c, o, defect, G=3):
    """The case's output with one defect, for 3 x 3 stride-1 cases of at least 2 channel tiles, 2 images and 2 G full tiles; G: workgroups of the walk.
      prev_ct_weights     the first step of tile 1 (channel tile 1) multiplied with channel tile 0's weights
      prev_image_film     the first tile of image 1 scaled / shifted with image 0's vectors (ebatch 1)
      next_tile_residual  tile 0 takes the residual of the workgroup's next tile G
      acc_not_cleared     tile G accumulates on top of tile 0
      src1_from_src0      the first chunk of src1 read from src0
      oob_row_pixel0      the row above image 0 read as pixel 0 instead of zero
      silu_border_only    the staged SiLU reaches only the pixels next to the zero padding
      bt_sign_row         B^T row 1 = [0 1 -1 0]                      (Winograd)
      drop_plane          plane 5 of the sixteen is not accumulated   (Winograd)"""
    g, gemm_n, Ho, Wo = case_geometry(c)
    kc, tn = g['kc'], g['tn']
    assert c['ks'] == 3 and c['st'] == 1 and g['nct'] >= 2 and c['N'] >= 2 and g['tiles'] >= 2 * G and Ho % g['th'] == 0 and Wo % g['tw'] == 0
    xs = [x.clone() for x in o['xs']]
    es, et, res, w = o['es'], case_et(o), o['res'], o['w']

    def region(t):
        n, ct, oy, ox = decode(t, g)
        return n, slice(oy, oy + g['th']), slice(ox, ox + g['tw']), slice(ct * tn, (ct + 1) * tn)
    if defect == 'src1_from_src0':
        xs[1][..., :kc] = xs[0][..., :kc]
    x = torch.cat(xs, 3)
    a = silu64(x) if c['pre'] else x
    if defect == 'silu_border_only':
        assert c['pre']
        a = x.clone()
        m = torch.zeros(x.shape[1], x.shape[2], dtype=torch.bool)
        m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
        a[:, m] = silu64(x[:, m])
    if defect == 'oob_row_pixel0':
        xp = pad1(a, 3)
        xp[0, 0, 1:-1, :] = a[0, 0, 0, :]
        z = conv_nhwc(xp, w, 3, 1, padded=True)
    elif defect == 'bt_sign_row':
        z = wino_forward(a, w, False, bt=(BT[0], (0, 1, -1, 0), BT[2], BT[3]))
    elif defect == 'drop_plane':
        z = wino_forward(a, w, False, drop_plane=5)
    else:
        z = conv_nhwc(a, w, 3, 1)
    if defect == 'prev_ct_weights':
        n, ys, xs_, cs = region(1)
        assert decode(1, g)[1] == 1
        a1 = a.clone()
        a1[..., kc:] = 0.0
        z1 = conv_nhwc(a1, w, 3, 1)
        z[n, ys, xs_, cs] += z1[n, ys, xs_, 0:tn] - z1[n, ys, xs_, cs]
    if defect == 'acc_not_cleared':
        n0, y0, x0, c0 = region(0)
        n1, y1, x1, c1 = region(G)
        z[n1, y1, x1, c1] += z[n0, y0, x0, c0]
    if defect == 'next_tile_residual':
        n0, y0, x0, c0 = region(0)
        n1, y1, x1, c1 = region(G)
        res = res.clone()
        res[n0, y0, x0, c0] = o['res'][n1, y1, x1, c1]
    y = epilogue(0.0, z, es, et, c['slope'], res)[0]
    if defect == 'prev_image_film':
        t = g['nct'] * g['ntx'] * g['nty']                      # first tile of image 1
        n, ys, xs_, cs = region(t)
        assert n == 1 and es is not None and es.shape[0] == c['N']
        y_alt = epilogue(0.0, z, es.roll(1, 0), et.roll(1, 0), c['slope'], res)[0]
        y[n, ys, xs_, cs] = y_alt[n, ys, xs_, cs]
    return y
