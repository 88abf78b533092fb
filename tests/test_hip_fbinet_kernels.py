"""GPU: the four entries of csrc/fbinet.hip (first, tapconv, rm, out) and yond_vst_minmax_f32, each alone against a float64 model, element
by element.  The bounds are derived, not measured.  u = 2^-24, gamma(k) = k u / (1 - k u):

  a chain of K fused multiply-adds (the fp32-input MFMA, fmaf) followed by the bias addition and a PReLU's multiplication differs from
  the exact value by at most  gamma(K + 4) (sum |w_i x_i| + |b|)  (K + 2 roundings; 2 spare), whatever the order of the chain;
  PReLU(.; s) has the Lipschitz factor max(1, |s|), halving 1/2; a value formed from ROUNDED operands adds their bounds times its
  own Lipschitz factors plus its own roundings (gamma(2) of the magnitudes that are added).

Operands are heavy-tailed (Student t, 3 degrees of freedom: tests/edge_model._ht), slopes negative, zero and positive.  TINY = 2^-149 per
rounding covers subnormal results."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fbinet_common as D
from edge_model import _ht

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
TINY = 2.0 ** -149
SHAPES = [(2, 2), (6, 10), (38, 50), (70, 132)]
LIVE = {0: ([(0, 1), (0, 3), (1, 0), (1, 4), (2, 2), (3, 0), (3, 4), (4, 1), (4, 3)], 5, 1, 2),      # taps (row, column), kernel, dilation, pad
        1: ([(0, 0), (0, 2), (1, 1), (2, 0), (2, 2)], 3, 3, 3)}


def gamma(k):
    return k * U / (1.0 - k * U)


def lib_():
    from yond_public_amd import _lib as L
    return L, L.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def slopes(r, c):
    """Per-channel slopes: negative, zero and positive ones in every 4 neighbouring channels, one above 1."""
    s = np.tile(np.array([-0.25, 0.0, 0.3, 0.1], np.float32), c // 4) * r.uniform(0.5, 1.5, c).astype(np.float32)
    s[c // 2] = 1.5
    return s


def prelu(x, s):
    return np.where(x > 0, x, x * s)


def lip(s):
    return np.maximum(1.0, np.abs(s.astype(np.float64)))


def tile():
    L, lib = lib_()
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    L.check(lib.yond_fbi_tile(ctypes.byref(th), ctypes.byref(tw)), "yond_fbi_tile")
    return th.value, tw.value


def named_pixels(H, W):
    """Every frame corner and each side of every tile seam (rows and columns), by name."""
    th, tw = tile()
    ys = sorted({0, H - 1} | {y for k in range(1, H // th + 1) for y in (k * th - 1, k * th) if y < H})
    xs = sorted({0, W - 1} | {x for k in range(1, W // tw + 1) for x in (k * tw - 1, k * tw) if x < W})
    return [(f"pixel ({y}, {x})" + (" corner" if y in (0, H - 1) and x in (0, W - 1) else " seam"), y, x) for y in ys for x in xs]


def check(name, got, want, bound, H=None, W=None):
    got = got.astype(np.float64)
    err = np.abs(got - want)
    assert np.isfinite(got).all()
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"[fbinet] {name}: max |err| {err.max():.3e}, largest err / bound {worst:.3f}, max |value| {np.abs(want).max():.3e}")
    assert (err <= bound).all(), name
    if H is not None:
        g, w_, b = (a.reshape(-1, H, W, a.shape[-1]) for a in (got, want, bound))
        for label, y, x in named_pixels(H, W):
            assert (np.abs(g[:, y, x] - w_[:, y, x]) <= b[:, y, x]).all(), f"{name}: {label}"


# ---------------------------------------------------------------------------------------------------------------------------
# tapconv
# ---------------------------------------------------------------------------------------------------------------------------
def tap_model(n_in, w, tset):
    """float64: (sum over the live taps of W_t n(. + d_t), the same sum of magnitudes); zero border."""
    taps, K, dil, pad = LIVE[tset]
    N, H, W, C = n_in.shape
    xp = np.pad(n_in.astype(np.float64), ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    acc, mag = np.zeros((N, H, W, C)), np.zeros((N, H, W, C))
    for r, c in taps:
        dy, dx = (r - K // 2) * dil, (c - K // 2) * dil
        sl = xp[:, pad + dy:pad + dy + H, pad + dx:pad + dx + W, :]
        wt = w[:, :, r, c].T.astype(np.float64)
        acc += sl @ wt
        mag += np.abs(sl) @ np.abs(wt)
    return acc, mag


@pytest.mark.parametrize("nf", [32, 64])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("tset", [0, 1])
def test_tapconv_against_float64_model(tset, hw, N, nf):
    L, lib = lib_()
    H, W = hw
    taps, K, dil, pad = LIVE[tset]
    r = np.random.default_rng(1000 * tset + 100 * nf + 10 * N + H)
    n_in, o_in = _ht(r, N, H, W, nf), _ht(r, N, H, W, nf)
    w = (_ht(r, nf, nf, K, K) / np.sqrt(len(taps) * nf)).astype(np.float32)
    b, s1, s2 = _ht(r, nf) * 0.1, slopes(r, nf), slopes(r, nf)[::-1].copy()
    wpk = np.empty(len(taps) * nf * nf, np.float32)
    L.check(lib.yond_pack_fbi_tap_weight_f32(w.ctypes.data, nf, tset, wpk.ctypes.data), "pack")
    n_out = torch.full((N, H, W, nf), float('nan'), device=DEV)
    o_out = torch.full((N, H, W, nf), float('nan'), device=DEV)
    d = [dev(a) for a in (n_in, o_in, wpk, b, s1, s2)]             # (held until the kernel has run)
    L.check(lib.yond_fbi_tapconv_f32(L.ptr(d[0]), L.ptr(d[1]), tset, nf, L.ptr(d[2]), L.ptr(d[3]), L.ptr(d[4]), L.ptr(d[5]),
                                     N, H, W, L.ptr(n_out), L.ptr(o_out), L.stream()), "yond_fbi_tapconv_f32")
    torch.cuda.synchronize()
    acc, mag = tap_model(n_in, w, tset)
    Kc = len(taps) * nf
    n_ref = prelu(acc + b.astype(np.float64), s1.astype(np.float64))
    e_n = lip(s1) * (gamma(Kc + 4) * (mag + np.abs(b)) + 2 * TINY)
    o_ref = prelu((n_ref + o_in) / 2.0, s2.astype(np.float64))
    e_o = lip(s2) * (0.5 * e_n + gamma(2) * 0.5 * (np.abs(n_ref) + np.abs(o_in)) + 2 * TINY)
    check(f"tapconv set {tset} {N}x{H}x{W}x{nf} n'", n_out.cpu().numpy(), n_ref, e_n, H, W)
    check(f"tapconv set {tset} {N}x{H}x{W}x{nf} o'", o_out.cpu().numpy(), o_ref, e_o, H, W)


# ---------------------------------------------------------------------------------------------------------------------------
# first
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [32, 64])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("hw", SHAPES)
def test_first_against_float64_model(hw, N, nf):
    L, lib = lib_()
    H, W = hw
    r = np.random.default_rng(7 + 100 * nf + 10 * N + H)
    x = _ht(r, N, 1, H, W)
    w = (_ht(r, nf, 1, 3, 3) / np.sqrt(8)).astype(np.float32)
    b = _ht(r, nf) * 0.1
    for slope in (-0.2, 0.0, 0.35):
        s = np.array([slope], np.float32)
        wpk = np.empty(8 * nf, np.float32)
        L.check(lib.yond_pack_fbi_first_weight_f32(w.ctypes.data, nf, wpk.ctypes.data), "pack")
        out = torch.full((N, H, W, nf), float('nan'), device=DEV)
        x4 = D.to_packed(torch.from_numpy(x)).to(DEV)
        d = [dev(a) for a in (wpk, b, s)]
        L.check(lib.yond_fbi_first_f32(L.ptr(x4), N, H // 2, W // 2, nf, L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), L.ptr(out), L.stream()),
                "yond_fbi_first_f32")
        torch.cuda.synchronize()
        xp = np.pad(x[:, 0].astype(np.float64), ((0, 0), (1, 1), (1, 1)))
        acc, mag = np.zeros((N, H, W, nf)), np.zeros((N, H, W, nf))
        for ky in range(3):
            for kx in range(3):
                if (ky, kx) == (1, 1):
                    continue                                        # the masked centre: the blind spot
                sl = xp[:, ky:ky + H, kx:kx + W, None]
                acc += sl * w[:, 0, ky, kx].astype(np.float64)
                mag += np.abs(sl) * np.abs(w[:, 0, ky, kx].astype(np.float64))
        ref = prelu(acc + b.astype(np.float64), float(s[0]))
        bound = max(1.0, abs(float(s[0]))) * (gamma(8 + 4) * (mag + np.abs(b)) + 2 * TINY)
        check(f"first {N}x{H}x{W} -> {nf}, slope {slope}", out.cpu().numpy(), ref, bound, H, W)


# ---------------------------------------------------------------------------------------------------------------------------
# rm
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [32, 64])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("mode, pre", [(1, False), (2, False), (0, True), (2, True)])
def test_rm_against_float64_model(mode, pre, hw, N, nf):
    """Write, accumulate, and the prologue form (v = PReLU(v / L; s): a correctly rounded float32 division and one multiplication,
    restated exactly in float32 here, so the model starts from the kernel's own v)."""
    L, lib = lib_()
    H, W = hw
    npix = N * H * W
    r = np.random.default_rng(31 + 1000 * mode + 100 * nf + 10 * N + H + int(pre))
    v = _ht(r, npix, nf)
    w1, w2 = ((_ht(r, nf, nf) / np.sqrt(nf)).astype(np.float32) for _ in range(2))
    b1, b2, a1, a2 = _ht(r, nf) * 0.1, _ht(r, nf) * 0.1, slopes(r, nf), slopes(r, nf)[::-1].copy()
    ps, layers = slopes(r, nf), 17
    sum0 = _ht(r, npix, nf)
    p1, p2 = np.empty(nf * nf, np.float32), np.empty(nf * nf, np.float32)
    L.check(lib.yond_pack_fbi_rm_weight_f32(w1.ctypes.data, nf, p1.ctypes.data), "pack")
    L.check(lib.yond_pack_fbi_rm_weight_f32(w2.ctypes.data, nf, p2.ctypes.data), "pack")
    o_out = torch.full((npix, nf), float('nan'), device=DEV)
    total = dev(sum0.copy())
    d = [dev(a) for a in (v, p1, b1, a1, p2, b2, a2, ps)]
    L.check(lib.yond_fbi_rm_f32(L.ptr(d[0]), nf, L.ptr(d[1]), L.ptr(d[2]), L.ptr(d[3]), L.ptr(d[4]), L.ptr(d[5]), L.ptr(d[6]),
                                L.ptr(d[7]) if pre else None, layers if pre else 0, npix, L.ptr(o_out), L.ptr(total) if mode else None, mode,
                                L.stream()), "yond_fbi_rm_f32")
    torch.cuda.synchronize()
    if pre:
        q = v / np.float32(layers)
        v = np.where(q > 0, q, q * ps).astype(np.float32)
    v64, W1, W2 = v.astype(np.float64), w1.astype(np.float64), w2.astype(np.float64)
    h_ref = prelu(v64 @ W1.T + b1, a1.astype(np.float64))
    e_h = lip(a1) * (gamma(nf + 4) * (np.abs(v64) @ np.abs(W1).T + np.abs(b1)) + 2 * TINY)
    r_ref = h_ref @ W2.T + b2
    e_r = gamma(nf + 4) * (np.abs(h_ref) @ np.abs(W2).T + np.abs(b2)) + (1 + gamma(nf + 4)) * (e_h @ np.abs(W2).T)
    o_ref = prelu((v64 + r_ref) / 2.0, a2.astype(np.float64))
    e_o = lip(a2) * (0.5 * e_r + gamma(2) * 0.5 * (np.abs(v64) + np.abs(r_ref)) + 2 * TINY)
    tag = f"rm mode {mode} prologue {pre} {N}x{H}x{W}x{nf}"
    check(tag + " o", o_out.cpu().numpy(), o_ref, e_o, H, W)
    if mode == 1:
        assert np.array_equal(total.cpu().numpy(), o_out.cpu().numpy())
    elif mode == 2:
        check(tag + " sum", total.cpu().numpy(), sum0 + o_ref, e_o + U * (np.abs(sum0) + np.abs(o_ref) + e_o) + TINY, H, W)
    else:
        assert np.array_equal(total.cpu().numpy(), sum0)


# ---------------------------------------------------------------------------------------------------------------------------
# out
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [32, 64])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("oc, sig", [(2, 0), (2, 1), (1, 0), (1, 1)])
def test_out_against_float64_model(oc, sig, hw, N, nf):
    """y = W f + b in any order of nf products: gamma(nf + 4) (sum |w f| + |b|).  sigmoid_value * sigmoid(y0): Lipschitz sv / 4, expf and the
    division within 8 u of the result (expf is held to 2 ulp elsewhere in this suite; two more roundings follow it).  a x + b is one fmaf."""
    L, lib = lib_()
    H, W = hw
    r = np.random.default_rng(77 + 1000 * oc + 100 * nf + 10 * N + H + sig)
    f = _ht(r, N, H, W, nf)
    w = (_ht(r, oc, nf) / np.sqrt(nf)).astype(np.float32)
    b = _ht(r, oc) * 0.1
    x = _ht(r, N, 1, H, W)
    sv = np.float32(0.1)
    x4 = D.to_packed(torch.from_numpy(x)).to(DEV)
    dst = torch.full((N, H // 2, W // 2, 4), float('nan'), device=DEV)
    d = [dev(a) for a in (f, w, b)]
    L.check(lib.yond_fbi_out_f32(L.ptr(d[0]), nf, L.ptr(d[1]), L.ptr(d[2]), oc, sig, float(sv), L.ptr(x4) if oc == 2 else None, N, H // 2, W // 2,
                                 L.ptr(dst), L.stream()), "yond_fbi_out_f32")
    torch.cuda.synchronize()
    f64 = f.astype(np.float64)
    y = f64 @ w.astype(np.float64).T + b
    e = gamma(nf + 4) * (np.abs(f64) @ np.abs(w.astype(np.float64)).T + np.abs(b)) + 2 * TINY
    y0, e0 = y[..., 0], e[..., 0]
    if sig:
        e0 = float(sv) * (e0 / 4.0 + 8 * U)
        y0 = float(sv) / (1.0 + np.exp(-y0))
    if oc == 2:
        xs = x[:, 0].astype(np.float64)
        ref = y0 * xs + y[..., 1]
        bound = np.abs(xs) * e0 + e[..., 1] + gamma(2) * (np.abs(y0 * xs) + np.abs(y[..., 1])) + TINY
    else:
        ref, bound = y0, e0
    got = D.from_packed(dst.cpu())[:, 0].numpy()
    check(f"out oc {oc} sigmoid {sig} {N}x{H}x{W}x{nf}", got[..., None], ref[..., None], bound[..., None], H, W)


# ---------------------------------------------------------------------------------------------------------------------------
# yond_vst_minmax_f32
# ---------------------------------------------------------------------------------------------------------------------------
def bias_form(form, K, s, mx):
    from yond_public_amd import pipeline as P
    if form == 'none':
        return None
    if form == 'knots':
        return P.get_bias(np.float32(mx) * np.float32(959.0), np.float64(s), np.float64(K), device=torch.device(DEV))
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "biaslut.npz"))
    row = P.BiasLUT(table=g["table"], x_lut=g["x_lut"], sg_lut=g["sg_lut"]).row(np.float64(K), np.float64(s), torch.device(DEV))
    assert row is not None
    return row


@pytest.mark.parametrize("hw", [(2, 2), (6, 10), (96, 128)])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("form", ['none', 'knots', 'row'])
def test_vst_minmax_equals_what_k1_normalises(form, B, hw):
    """The entry's (min, max) against K1 itself.  K1 clamps its output to [0, 1] and the stabilised value is never below 2 sqrt(3/8) = 1.22,
    so with lower = 0, upper = 1 K1 would store 1.0 everywhere; the span is therefore a power of two that holds every value, lower = 0,
    upper = 64: (v - 0) * 2^-6 is exact in float64 and the one rounding to float32 commutes with it, so 64 * K1's output IS float32(v), bit
    for bit, and its torch.min / torch.max must equal the entry's two float64 numbers rounded to float32 (rounding is monotonic), bit for
    bit.  p2d = 0, the three bias forms, one frame and a stack of 3.  Then K1 with the entry's own bounds: extremes exactly 0 and 1."""
    from yond_public_amd import pipeline as P
    L, lib = lib_()
    H, W = hw
    K, s = 4.37, 6.27
    frames = np.stack([D.synth_noisy(H, W, K, s, 200 + i)[0] * np.float32(0.5 + 0.25 * i) for i in range(B)])
    f = bias_form(form, K, s, float(frames.max()))
    lut_n = 0 if f is None else len(f)
    two_d = int(f is not None and isinstance(f, P.DeviceBiasRow))
    fr = dev(frames)
    mm = torch.full((B, 2), float('nan'), dtype=torch.float64, device=DEV)
    L.check(lib.yond_vst_minmax_f32(L.ptr(fr), B, H, W, 959.0, K, s, L.ptr(f.x) if lut_n else None, L.ptr(f.y) if lut_n else None, lut_n, two_d,
                                    L.ptr(mm), L.stream()), "yond_vst_minmax_f32")
    mm = mm.cpu().numpy()

    def k1(i, lo, hi):
        out = torch.full((H // 2, W // 2, 4), float('nan'), device=DEV)
        if two_d:
            L.check(lib.yond_pack_vst_norm_biaslut_f32(L.ptr(fr[i]), H, W, L.ptr(out), 0, 0, 0, 0, 959.0, K, s, lo, hi, L.ptr(f.x), L.ptr(f.y), lut_n,
                                                       None, L.stream()), "yond_pack_vst_norm_biaslut_f32")
        else:
            L.check(lib.yond_pack_vst_norm_f32(L.ptr(fr[i]), H, W, L.ptr(out), 0, 0, 0, 0, 1, 959.0, K, s, lo, hi, L.ptr(f.x) if lut_n else None,
                                               L.ptr(f.y) if lut_n else None, lut_n, None, L.stream()), "yond_pack_vst_norm_f32")
        return out

    for i in range(B):
        v32 = k1(i, 0.0, 64.0) * 64.0
        assert float(v32.max()) < 64.0 and float(v32.min()) > 0.0          # (no clamp was reached)
        print(f"[fbinet] minmax {form} frame {i} of {B} {H}x{W}: entry ({mm[i, 0]!r}, {mm[i, 1]!r}), K1 ({float(v32.min())!r}, {float(v32.max())!r})")
        assert np.float32(mm[i, 0]).tobytes() == np.float32(v32.min().item()).tobytes()
        assert np.float32(mm[i, 1]).tobytes() == np.float32(v32.max().item()).tobytes()
        unit = k1(i, float(mm[i, 0]), float(mm[i, 1]))
        assert float(unit.min()) == 0.0 and float(unit.max()) == 1.0
    if B > 1:
        assert len({mm[i, 1] for i in range(B)}) == B                       # (the frames differ: a per-frame result, not the stack's)
