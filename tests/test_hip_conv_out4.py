"""GPU: yond_conv3x3_out4_f32 (csrc/conv3x3_out4.hip, the last layer of DnCNN) against a float64 model, element by element.

The bound follows the kernel's accumulation order, with the conventions of tests/fp32_model.py (u = 2^-24; an fp32 MFMA is a chain of
fused multiply-adds, one rounding of the accumulator per product; roundings walk randomly; the tests assert err <= FACTOR * T):
  * per output and tap column dx one accumulator T_dx = sum over (dy, ci) of w a: a chain of K = 3 Cin products (rows outside the image
    add exact zeros, counted all the same):     sqrt(K) u (Q_dx + |T_dx|),   Q_dx = sqrt(sum (w a)^2);   the three chains independent: RSS;
  * s = (T_0 + T_1) + T_2: two roundings, u |T_0 + T_1| + u |s|;
  * o = s + bias: u |o| (none without a bias: the kernel adds an exact zero);
  * y = x + sign o: u |y| (none without x: the sign is exact);
  * a result in the subnormal range: + 2^-149.
The operands are exact float32 of any magnitude: nothing is rounded to half, so values beyond fp16's range must hold the same bound."""
import ctypes as C

import numpy as np
import pytest
import torch

import fp32_model as FM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24

#        N  H   W    Cin
SHAPES = {1: (1, 5, 7, 16),        # smaller than any tile; every pixel on a border
          2: (2, 33, 70, 64),      # crosses the row bands (6 rows at this size: 4 steps) and the 62-column segments; two images
          3: (1, 16, 130, 128),    # three segments, the last 6 columns wide; the widest channel count
          # the band height follows the number of workgroups (band_steps below): many small images reach the taller bands cheaply
          4: (512, 28, 7, 16),     # 14-row bands (8 steps), two per image
          5: (512, 60, 7, 16),     # 30-row bands (16 steps), two per image
          6: (512, 44, 7, 16)}     # 22-row bands (12 steps), two per image


def band_steps(N, H, W):
    """The host's choice restated (yond_conv3x3_out4_f32): steps of two input rows per band, a band = 2 * steps - 2 output rows -- the even
    step count 4 .. 16 with the smallest steps x (workgroups of four (segment, band, image) items on the busiest of 256 CUs), the tallest
    band among equals."""
    nseg = (W + 61) // 62
    cost = lambda st: st * (((nseg * ((H + 2 * st - 3) // (2 * st - 2)) * N + 3) // 4 + 255) // 256)
    return min(range(16, 3, -2), key=cost)


def pack(w):
    """w [4][Cin][3][3] (device) through the host packer -> the kernel's weights on the device."""
    from yond_public_amd import _lib as L
    wn = np.ascontiguousarray(w.cpu().numpy().astype(np.float32))
    packed = np.empty(wn.size, np.float32)
    L.check(L.load().yond_pack_conv3x3_out4_weight_f32(wn.ctypes.data, wn.shape[1], packed.ctypes.data), "yond_pack_conv3x3_out4_weight_f32")
    return torch.from_numpy(packed).to(DEV)


def run_kernel(feat, w, bias, x, sign):
    from yond_public_amd import _lib as L
    lib = L.load()
    N, H, W, Cin = feat.shape
    wd = pack(w)
    dst = torch.full((N, H, W, 4), float('nan'), dtype=torch.float32, device=DEV)
    L.check(lib.yond_conv3x3_out4_f32(L.ptr(feat), Cin, L.ptr(wd), L.ptr(bias), L.ptr(x), float(sign), N, H, W, L.ptr(dst), L.stream()),
            "yond_conv3x3_out4_f32")
    torch.cuda.synchronize()
    return dst


def model(feat, w, bias, x, sign):
    """(y, T) in float64 on the tensors' device: feat [N][H][W][Cin], w [4][Cin][3][3]."""
    a, w64 = feat.double(), w.double()
    ap = FM.pad1(a, 3)
    N, H, W, Cin = a.shape
    cols, rss = [], 0.0
    for dx in range(3):
        t = q2 = 0.0
        for dy in range(3):
            s = ap[:, dy:dy + H, dx:dx + W, :]
            wt = w64[:, :, dy, dx].t()
            t = t + s @ wt
            q2 = q2 + (s * s) @ (wt * wt)
        cols.append(t)
        rss = rss + (np.sqrt(3 * Cin) * U * (q2.sqrt() + t.abs())) ** 2
    s01 = cols[0] + cols[1]
    s = s01 + cols[2]
    T = rss.sqrt() + U * s01.abs() + U * s.abs()
    o = s
    if bias is not None:
        o = s + bias.double()
        T = T + U * o.abs()
    y = sign * o
    if x is not None:
        y = x.double() + y
        T = T + U * y.abs()
    return y, T + FM.TINY


def operands(case, kind, seed):
    N, H, W, Cin = SHAPES[case]
    rng = np.random.default_rng(seed)
    a = FM.stress_acts(rng, (N, Cin, H, W), kind)
    if kind == 'beyond':
        # (stress_acts replaces about 1e-3 of the elements: the smallest shape may get none -- four more, isolated, 1e5 .. 1e6, both signs)
        for i in rng.choice(a.size, 4, replace=False):
            a.reshape(-1)[i] = 10.0 ** rng.uniform(5.0, 6.0) * rng.choice([-1.0, 1.0])
    feat = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 3, 1))).to(DEV)
    w = torch.from_numpy(FM.stress_weights(rng, 4, Cin, 3, kind)).to(DEV)
    bias = torch.from_numpy((rng.standard_normal(4) * (1e3 if kind == 'beyond' else 1.0)).astype(np.float32)).to(DEV)
    x = torch.from_numpy(rng.standard_normal((N, H, W, 4)).astype(np.float32)).to(DEV)
    return feat, w, bias, x


def check(name, got, y, T):
    err = (got.double() - y).abs()
    ratio = float((err / T).max())
    print(f"[out4] {name}: max err / T = {ratio:.3f}, max |y| = {float(y.abs().max()):.3e}, max err = {float(err.max()):.3e}")
    assert bool(torch.isfinite(got).all())
    assert ratio <= FM.FACTOR, name


@pytest.mark.parametrize("case", [1, 2, 3])
@pytest.mark.parametrize("kind", ["tame", "signed", "beyond"])
def test_out4_matches_float64_model(case, kind):
    """Every combination of bias / x / sign on one set of operands per (shape, operand kind); 'beyond' holds activations up to 1e6 and weights
    up to 2e5 -- far outside fp16's range."""
    feat, w, bias, x = operands(case, kind, 100 * case + len(kind))
    if kind == 'beyond':
        assert float(feat.abs().max()) > 65504.0 and float(w.abs().max()) > 65504.0
    for use_bias in (False, True):
        for use_x in (False, True):
            for sign in (1.0, -1.0):
                b, xx = (bias if use_bias else None), (x if use_x else None)
                got = run_kernel(feat, w, b, xx, sign)
                y, T = model(feat, w, b, xx, sign)
                check(f"case {case} {kind} bias={use_bias} x={use_x} sign={sign:+.0f}", got, y, T)


@pytest.mark.parametrize("case,steps", [(4, 8), (5, 16), (6, 12)])
def test_out4_taller_bands(case, steps):
    """The taller bands the kernel takes once the launch fills the chip: heavy-tailed operands, bias, residual, sign -1; and a NaN next to a
    band seam stays in its footprint."""
    N, H, W, Cin = SHAPES[case]
    assert band_steps(N, H, W) == steps and band_steps(*SHAPES[2][:3]) == 4
    feat, w, bias, x = operands(case, 'signed', 40 + case)
    got = run_kernel(feat, w, bias, x, -1.0)
    y, T = model(feat, w, bias, x, -1.0)
    check(f"case {case} ({2 * steps - 2}-row bands)", got, y, T)
    seam = 2 * steps - 2                                       # first row of the second band
    f2 = feat.clone()
    f2[N // 2, seam, 3, 5] = float('nan')
    got2 = run_kernel(f2, w, bias, x, -1.0)
    inside = torch.zeros((N, H, W), dtype=torch.bool, device=DEV)
    inside[N // 2, seam - 1:seam + 2, 2:5] = True
    assert torch.equal(got2[~inside], got[~inside]) and bool(torch.isnan(got2[inside]).all())


def test_out4_model_bound_catches_defects():
    """The bound is tight enough to see a lost tap, a lost channel and a wrong sign (evaluated on the model alone, against the kernel's output)."""
    feat, w, bias, x = operands(2, 'tame', 7)
    got = run_kernel(feat, w, bias, x, -1.0)
    y, T = model(feat, w, bias, x, -1.0)
    assert float(((got.double() - y).abs() / T).max()) <= FM.FACTOR
    w_tap = w.clone()
    w_tap[:, :, 2, 0] = 0
    w_ch = w.clone()
    w_ch[:, 37] = 0
    for name, yy in (("tap", model(feat, w_tap, bias, x, -1.0)[0]), ("channel", model(feat, w_ch, bias, x, -1.0)[0]),
                     ("sign", model(feat, w, bias, x, 1.0)[0])):
        assert float(((got.double() - yy).abs() / T).max()) > 100 * FM.FACTOR, name


@pytest.mark.parametrize("case,pix", [(2, (1, 29, 61)), (2, (0, 0, 0)), (2, (1, 32, 69)), (3, (0, 7, 124)), (1, (0, 2, 3))])
def test_out4_nan_stays_inside_its_footprint(case, pix):
    """A NaN (and an infinity) planted in one input pixel reaches exactly the outputs whose 3x3 window holds that pixel -- across band and
    segment seams, too; every other output keeps the bits of the clean run."""
    feat, w, bias, x = operands(case, 'tame', 11)
    clean = run_kernel(feat, w, bias, x, -1.0)
    n, py, px = pix
    N, H, W, Cin = feat.shape
    for bad in (float('nan'), float('inf')):
        f2 = feat.clone()
        f2[n, py, px, Cin // 2] = bad
        got = run_kernel(f2, w, bias, x, -1.0)
        inside = torch.zeros((N, H, W), dtype=torch.bool, device=DEV)
        inside[n, max(py - 1, 0):py + 2, max(px - 1, 0):px + 2] = True
        assert bool(torch.isfinite(got[~inside]).all())
        assert torch.equal(got[~inside], clean[~inside])
        assert not bool(torch.isfinite(got[inside]).all(dim=-1).any())      # (tame weights are non-zero: every window that holds the pixel shows it)


def test_out4_does_not_write_outside_the_image():
    """The destination sits inside a larger buffer of sentinels; the rows before and after it keep them."""
    feat, w, bias, x = operands(3, 'tame', 13)
    from yond_public_amd import _lib as L
    lib = L.load()
    N, H, W, Cin = feat.shape
    wd = pack(w)
    buf = torch.full((N * (H + 8) * W * 4,), 1234.5, dtype=torch.float32, device=DEV)
    dst = buf[4 * W * 4:4 * W * 4 + N * H * W * 4]
    L.check(lib.yond_conv3x3_out4_f32(L.ptr(feat), Cin, L.ptr(wd), None, None, 1.0, N, H, W, C.c_void_p(dst.data_ptr()), L.stream()), "out4")
    torch.cuda.synchronize()
    assert bool((buf[:4 * W * 4] == 1234.5).all()) and bool((buf[4 * W * 4 + N * H * W * 4:] == 1234.5).all())
    y, T = model(feat, w, None, None, 1.0)
    assert float(((dst.reshape(N, H, W, 4).double() - y).abs() / T).max()) <= FM.FACTOR
