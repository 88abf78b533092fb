"""GPU: every launch form of the split-operand kernels (csrc/conv_split_kernel.h, gemm_split.hip) on HARD operands -- heavy-tailed
weights, output channels whose scales differ by 10^4, dominant input channels, activations spread over 10^4 with many operands
below fp16's normal range or close to its maximum -- against a float64 reference, EVERY output element against a bound of its own:
|got - ref64| <= 4 T (tests/split_model.py; tests/test_split_model.py shows the arithmetic's model stays below 1 T and that a
single lost half, a wrong 2^-11 or flushed subnormals exceed 4 T).  Forms that store halves are scaled to max|output| ~ 3e4 and
must leave the range-guard word at 0; their planes must decode to the float32 output of the same launch form to 2^-22 |y| + 2^-36.
Forms that read split input take their reference from the decoded planes.  No case excludes outputs.
Every form has one case with an exactly zero input channel and an output channel whose weights are all zero: that channel must hold the
bias path BIT FOR BIT (a stored plane: the exact halves of it; behind a SiLU, whose device form has no bit-exact host twin: one value per
image, and the halves of that value)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import split_model as M
from test_hip_conv import (DEV, bare_plan, from_p4, hp_decode, nchw, nhwc, run_conv, sp_decode, sp_halves, to_hp, to_p4, to_sp)

pytestmark = pytest.mark.gpu


def T_(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def check(name, got, ref, T, ch_axis=1):
    r = M.ratio_report(name, got, ref, T, ch_axis)
    assert r.max() <= M.FACTOR, (name, float(r.max()))
    return float(r.max())


def exact_channel(name, got, want=None, pre=None):
    """The all-zero output channel, `got` [N][...] float32: equal to `want` bit for bit; or (behind a SiLU) one value per image, SiLU(pre [N])
    to the device SiLU's own error: 2^-21 for its exp2 / rcp / roundings, |pre| 2^-23 for the rounded exponent argument."""
    got = got.float()
    if want is not None:
        assert torch.equal(got, want.float().expand_as(got)), (name, float((got - want).abs().max()))
        return
    flat = got.reshape(got.shape[0], -1)
    assert bool((flat == flat[:, :1]).all()), name
    ref = F.silu(pre.double())
    assert bool(((flat[:, 0].double() - ref).abs() <= (2.0 ** -21 + pre.double().abs() * 2.0 ** -23) * ref.abs() + 2.0 ** -126).all()), name


def exact_halves(name, planes, y32, N, C, H, W, parts, c0):
    """Channel c0 of a stored plane tensor: exactly the halves of the float32 value y32 [N][H][W] (h = fp16(y), l = fp16((y - h) 2^11))."""
    h = y32.half()
    if parts == 2:
        gh, gl = sp_halves(planes, N, C, H, W)
        l = ((y32 - h.float()) * 2048.0).half()
        assert torch.equal(gh[..., c0].view(torch.int16), h.view(torch.int16)) and torch.equal(gl[..., c0].view(torch.int16), l.view(torch.int16)), name
    else:
        gh, _ = hp_decode(planes, N, C, H, W)
        assert torch.equal(gh[..., c0].view(torch.int16), h.view(torch.int16)), name


def plan_with_status():
    plan = bare_plan()
    plan.status, plan.status_slot = torch.zeros(4, dtype=torch.int32, device=DEV), 0
    return plan


def scale_to(w, y_lin, target=3.0e4):
    """One global factor on the weights so that max|output| ~ target (the output is linear in w up to the FiLM shift)."""
    f = target / float(y_lin.abs().max())
    f = min(f, 6.0e4 / float(np.abs(w).max()))
    return (w * np.float32(f)).astype(np.float32)


def operands(seed, C, Co, N, H, W, kind, zero, film, k=3):
    rng = np.random.default_rng([seed, C, Co, H, W])
    x = M.stress_acts(rng, (N, C, H, W), kind, zero_ch=3 if zero else None)
    w = M.stress_weights(rng, Co, C, k, zero_out=Co - 2 if zero else None)
    if film:
        es, et = M.stress_film(rng, N, Co)
    else:
        es, et = None, (10.0 ** rng.uniform(-2, 2, Co) * rng.choice([-1.0, 1.0], Co)).astype(np.float32)
    return rng, x, w, es, et


def epilogue(Tz, z, es, et, post, slope, res, half_out=False):
    """(y, T_y) for NCHW z; es / et: [N][Co] FiLM or None / [Co] bias."""
    sc = None if es is None else T_(es).double()[:, :, None, None]
    sh = T_(et).double()[:, :, None, None] if et.ndim == 2 else T_(et).double()[None, :, None, None]
    return M.through_epilogue(Tz, z, sc, sh, post, slope, res, half_out)


def make_res(rng, p):
    """A residual of the output's own magnitude (float32)."""
    return (p.abs() * T_(rng.standard_normal(tuple(p.shape)))).float()


def film_kw(es, et, pre, post, slope):
    kw = dict(pre_act=pre, post_act=post, slope=slope)
    if es is not None:
        kw.update(escale=T_(es).to(DEV), eshift=T_(et).to(DEV), ebatch=1)
    return kw


# ---- 3x3 layers on [N][H][W][C] float32 tensors ------------------------------------------------------------------------------

NHWC_CASES = [
    # name, C (or (C0, C1)), Co, N, H, W, stride, kind, film, pre, post, res, zero
    ("s1 32 aligned", 32, 32, 1, 16, 64, 1, 'pos', False, 0, 0, False, False),
    ("s1 32 ragged", 32, 64, 1, 9, 33, 1, 'big', False, 0, 0, False, True),
    ("s1 64 aligned", 64, 64, 2, 16, 64, 1, 'signed', False, 0, 0, False, False),
    ("s1 64 ragged", 64, 32, 1, 17, 40, 1, 'pos', False, 0, 0, False, True),
    ("s1 128 aligned", 128, 128, 1, 8, 32, 1, 'big', False, 0, 0, False, False),
    ("s1 128 ragged", 128, 128, 1, 24, 40, 1, 'signed', False, 0, 0, False, True),
    ("s1 256 aligned", 256, 64, 1, 8, 32, 1, 'pos', False, 0, 0, False, False),
    ("s1 256 ragged", 256, 64, 1, 30, 61, 1, 'signed', False, 0, 0, False, True),
    ("12-row tiles aligned", 64, 64, 1, 192, 512, 1, 'signed', False, 0, 0, False, False),
    ("12-row tiles ragged, fused", 64, 64, 1, 188, 540, 1, 'pos', True, 1, 2, True, True),
    ("folded tiles aligned", 64, 64, 70, 16, 16, 1, 'signed', False, 0, 2, True, False),
    ("folded tiles ragged", 64, 128, 5, 13, 11, 1, 'pos', False, 0, 2, True, True),
    ("two-source aligned", (32, 32), 32, 1, 16, 32, 1, 'signed', False, 0, 2, False, False),
    ("two-source ragged", (32, 32), 32, 1, 17, 40, 1, 'big', False, 0, 2, False, True),
    ("FiLM + SiLU + residual aligned", 64, 64, 2, 16, 64, 1, 'signed', True, 1, 2, True, False),
    ("FiLM + SiLU + residual ragged", 64, 64, 2, 20, 48, 1, 'big', True, 1, 2, True, True),
    ("SiLU epilogue aligned", 64, 64, 2, 48, 96, 1, 'signed', True, 1, 1, False, False),
    ("SiLU epilogue ragged", 32, 32, 2, 40, 70, 1, 'pos', True, 1, 1, False, True),
    ("s2 aligned", 64, 128, 2, 32, 64, 2, 'signed', False, 0, 0, False, False),
    ("s2 ragged", 32, 64, 1, 18, 35, 2, 'big', False, 0, 0, False, True),
    ("s2 folded aligned", 64, 128, 40, 32, 32, 2, 'pos', False, 0, 0, False, False),
    ("s2 folded ragged", 64, 128, 70, 11, 13, 2, 'signed', False, 0, 0, False, True),
]


def nhwc_case(name, C, Co, N, H, W, stride, kind, film, pre, post, res, zero, parts=2, seed=1):
    splits = list(C) if isinstance(C, tuple) else [C]
    C = sum(splits)
    rng, x, w, es, et = operands(seed, C, Co, N, H, W, kind, zero, film)
    x64 = T_(x).double()
    a64 = F.silu(x64) if pre else x64
    z = F.conv2d(a64, T_(w).double(), stride=stride, padding=1)
    Tz = M.threshold_conv(a64, T_(w), z, stride, parts, pre_silu=bool(pre))
    slope = 0.3 if post == 2 else 0.0
    p, _ = epilogue(Tz, z, es, et, post, slope, None)
    r = make_res(rng, p) if res else None
    y, Ty = epilogue(Tz, z, es, et, post, slope, None if r is None else r.double())
    xs, off = [], 0
    for c in splits:
        xs.append(nhwc(T_(x[:, off:off + c])).to(DEV))
        off += c
    kw = film_kw(es, et, pre, post, slope)
    got = run_conv(T_(w), None if film else T_(et), 3, stride, splits, xs, N, H, W, algo='split' if parts == 2 else 'half',
                   res=None if r is None else nhwc(r).to(DEV), **kw)
    assert got.shape[-1] == Co                                     # (no padded channels in these layers: every element is checked)
    got = nchw(got).double()
    check(f"PARTS {parts} {name} [{kind}]", got, y, Ty)
    if zero:
        # the all-zero output channel: exactly the bias path, in float32
        c0 = Co - 2
        sh = T_(et)[:, c0][:, None, None] if film else T_(et)[c0]
        want = torch.zeros(N, *got.shape[2:]) + sh
        if post == 1:
            assert r is None
            exact_channel(name, got[:, c0], pre=want[:, 0, 0])
        else:
            want = F.leaky_relu(want, slope) if post == 2 else want
            exact_channel(name, got[:, c0], want + r[:, c0] if r is not None else want)


@pytest.mark.parametrize("case", NHWC_CASES, ids=[c[0].replace(' ', '_') for c in NHWC_CASES])
def test_split_nhwc_forms(case):
    nhwc_case(*case)


HALF_CASES = [
    ("staged aligned", 64, 64, 1, 16, 64, 1, 'signed', False, 0, 0, False, False),
    ("staged ragged, fused", 64, 64, 1, 24, 40, 1, 'pos', True, 1, 2, True, True),
    ("128-channel tiles aligned", 128, 128, 1, 16, 64, 1, 'pos', False, 0, 0, False, False),
    ("128-channel tiles ragged, fused", 64, 256, 2, 37, 70, 1, 'signed', True, 1, 0, True, True),
    ("s2 staged ragged", 32, 64, 1, 18, 35, 2, 'big', False, 0, 0, False, True),
]


@pytest.mark.parametrize("case", HALF_CASES, ids=[c[0].replace(' ', '_') for c in HALF_CASES])
def test_half_nhwc_forms(case):
    """precision='fp16' (PARTS 1, h halves only) on plain tensors, against the PARTS 1 bound."""
    nhwc_case(*case, parts=1)


# ---- the split-plane / h-only-plane data flow ---------------------------------------------------------------------------------

def decode_planes(buf, N, C, H, W, parts):
    """Planes -> ([N][C][H][W] float64, pads)."""
    if parts == 2:
        return sp_decode(buf, N, C, H, W)
    h, pads = hp_decode(buf, N, C, H, W)
    return nchw(h).double(), pads


def to_planes(x_nhwc, parts):
    return to_sp(x_nhwc) if parts == 2 else to_hp(x_nhwc)


def stored_as_halves(name, val, y32, parts):
    """A stored plane tensor against the float32 output of the same launch form: h + l 2^-11 to 2^-22 |y| + 2^-36 (h only: the
    half-rounding of y, bit for bit)."""
    y32 = y32.double()
    if parts == 2:
        d = (val - y32).abs()
        assert bool((d <= 2.0 ** -22 * y32.abs() + 2.0 ** -36).all()), (name, float(d.max()))
    else:
        assert torch.equal(val.float().half(), y32.float().half()), name


@pytest.mark.parametrize("parts", [2, 1])
@pytest.mark.parametrize("C,N,H,W,kind,in_p4", [(64, 2, 16, 64, 'signed', False), (32, 2, 37, 70, 'pos', True), (128, 1, 24, 40, 'signed', True),
                                                (64, 5, 16, 16, 'pos', True), (64, 3, 13, 11, 'signed', True)])
def test_planes_out(parts, C, N, H, W, kind, in_p4):
    """conv1 of a residual block: SiLU staging, FiLM, SiLU, stored as split planes (PARTS 1: h-only planes); input [N][H][W][C] or planes
    of 4 channels.  Plain and folded tiles."""
    from yond_public_amd.engine import _PackedConv
    rng, x, w, es, et = operands(2 + parts, C, C, N, H, W, kind, H == 37, True)
    a64 = F.silu(T_(x).double())
    z0 = F.conv2d(a64, T_(w).double(), padding=1)
    w = scale_to(w, z0 * T_(es).double()[:, :, None, None])
    z = F.conv2d(a64, T_(w).double(), padding=1)
    Tz = M.threshold_conv(a64, T_(w), z, 1, parts, pre_silu=True)
    y, Ty = epilogue(Tz, z, es, et, 1, 0.0, None, half_out=parts == 1)
    if parts == 2:
        Ty = Ty + 2.0 ** -22 * y.abs() + 2.0 ** -36
    plan = plan_with_status()
    pc = _PackedConv(plan.dev, T_(w), None, 3, 1, [C])
    kw = film_kw(es, et, 1, 1, 0.0)
    kw['algo'] = 'split' if parts == 2 else 'half'
    xn = nhwc(T_(x))
    out = plan._new_sp('t', N, H, W, C, parts)
    plan._conv(pc, to_p4(xn) if in_p4 else xn.to(DEV), None, N, H, W, out, in_fmt=2 if in_p4 else 0, out_fmt=1, **kw)
    y32 = torch.full((N, H, W, C), float('nan'), device=DEV)
    plan._conv(pc, xn.to(DEV), None, N, H, W, y32, **kw)
    torch.cuda.synchronize()
    assert int(plan.status[0]) == 0
    val, pads = decode_planes(out, N, C, H, W, parts)
    assert not pads.view(torch.int16).any()
    check(f"PARTS {parts} planes out C{C} {N}x{H}x{W} [{kind}]", val, y, Ty)
    stored_as_halves("planes out", val, nchw(y32.cpu()), parts)
    if H == 37:
        c0 = C - 2
        exact_channel("planes out, float32 twin", y32.cpu()[..., c0], pre=T_(et)[:, c0])
        exact_halves("planes out", out, y32.cpu()[..., c0], N, C, H, W, parts, c0)


PLANES_IN = [(64, 2, 16, 64, 'signed', False, False), (32, 2, 37, 70, 'pos', True, False), (128, 1, 24, 40, 'signed', True, False),
             (64, 3, 13, 11, 'pos', True, False), (32, 1, 37, 70, 'signed', False, True), (32, 1, 16, 64, 'pos', False, True)]


# (h-only planes in, float32 [N][H][W][C] out is not a launch form: the fp16 flow's conv2 stores planes or the output projection)
@pytest.mark.parametrize("parts,C,N,H,W,kind,out_planes,out4", [(2,) + c for c in PLANES_IN] + [(1,) + c for c in PLANES_IN if c[5] or c[6]])
def test_planes_in(parts, C, N, H, W, kind, out_planes, out4):
    """conv2 of a residual block: input in split planes (staged by LDS-DMA: the reference is computed from the decoded planes), FiLM +
    residual; output float32, split planes (residual in planes of 4), or the fused output projection."""
    from yond_public_amd.engine import _PackedConv
    zero = H == 37
    c0 = C - 2
    rng, x, w, es, et = operands(5 + parts, C, C, N, H, W, kind, zero, True)
    xn = nhwc(T_(x))
    xin = to_planes(xn, parts)
    a64, _ = decode_planes(xin, N, C, H, W, parts)
    if out_planes:
        w = scale_to(w, F.conv2d(a64, T_(w).double(), padding=1) * T_(es).double()[:, :, None, None])
    z = F.conv2d(a64, T_(w).double(), padding=1)
    Tz = M.threshold_conv(a64, T_(w), z, 1, parts)
    p, _ = epilogue(Tz, z, es, et, 0, 0.0, None)
    r = make_res(rng, p)
    if out_planes:
        r = r * 0.5                                                # (keeps max|output| below fp16's range)
    y, Ty = epilogue(Tz, z, es, et, 0, 0.0, r.double(), half_out=out_planes and parts == 1)
    plan = plan_with_status()
    pc = _PackedConv(plan.dev, T_(w), None, 3, 1, [C])
    kw = film_kw(es, et, 0, 0, 0.0)
    kw['algo'] = 'split' if parts == 2 else 'half'
    rn = nhwc(r)
    if out4:
        w4 = T_(M.stress_weights(rng, 4, C, 1)[:, :, 0, 0] / np.float32(100.0))
        b4 = T_(rng.standard_normal(4).astype(np.float32))
        x4 = T_(rng.random((N, H, W, 4)).astype(np.float32))
        ub = T_((rng.random(N) + 0.5).astype(np.float32))
        o4 = torch.full((N, H, W, 4), float('nan'), device=DEV)
        plan._conv(pc, xin, None, N, H, W, None, res=rn.to(DEV), in_fmt=1, out4=(w4.to(DEV), b4.to(DEV), x4.to(DEV), ub.to(DEV), o4), **kw)
        torch.cuda.synchronize()
        if zero:
            # the projection of the all-zero channel ALONE (every other projection weight zero, no input residual, no de-normalisation): every
            # other term of its sum is an exact zero, so the output is w4 * (shift + res) + b4 in float32 -- one product and one sum, fused or not
            w40 = torch.zeros_like(w4)
            w40[:, c0] = w4[:, c0]
            o40 = torch.full((N, H, W, 4), float('nan'), device=DEV)
            plan._conv(pc, xin, None, N, H, W, None, res=rn.to(DEV), in_fmt=1, out4=(w40.to(DEV), b4.to(DEV), None, None, o40), **kw)
            torch.cuda.synchronize()
            f0 = (T_(et)[:, c0][:, None, None] + rn[..., c0])[..., None]                     # [N][H][W][1] float32: the bias path
            plain = f0 * w40[:, c0] + b4
            fused = (f0.double() * w40[:, c0].double() + b4.double()).float()               # (a float32 product is exact in float64: one rounding)
            assert torch.equal(o40.cpu(), plain) or torch.equal(o40.cpu(), fused), float((o40.cpu() - plain).abs().max())
        u = ub.double()[:, None, None, None]
        yn, Tn = nhwc(y), nhwc(Ty)
        lin = torch.einsum('nhwc,qc->nhwq', yn, w4.double())
        mag = torch.einsum('nhwc,qc->nhwq', yn.abs(), w4.double().abs()) + b4.double().abs() + (x4.double() / u).abs()
        want = (lin + b4.double() + x4.double() / u) * u
        # the projection is a float32 sum of C + 2 terms and one product: at most (C + 3) roundings of the terms' magnitude
        T4 = u * (torch.einsum('nhwc,qc->nhwq', Tn, w4.double().abs()) + 2.0 ** -24 * (C + 3) * mag)
        check(f"PARTS {parts} planes in + output projection C{C} {H}x{W} [{kind}]", o4.cpu(), want, T4, ch_axis=3)
        return
    if out_planes:
        out = plan._new_sp('o', N, H, W, C, parts)
        plan._conv(pc, xin, None, N, H, W, out, res=to_p4(rn), in_fmt=1, out_fmt=1, res_fmt=2, **kw)
        torch.cuda.synchronize()
        assert int(plan.status[0]) == 0
        val, pads = decode_planes(out, N, C, H, W, parts)
        assert not pads.view(torch.int16).any()
        check(f"PARTS {parts} planes in and out C{C} {N}x{H}x{W} [{kind}]", val, y,
              Ty + (2.0 ** -22 * y.abs() + 2.0 ** -36 if parts == 2 else 0.0))
        if zero:
            exact_halves("planes in and out", out, T_(et)[:, c0][:, None, None] + rn[..., c0], N, C, H, W, parts, c0)
    if parts == 1:
        return
    y32 = torch.full((N, H, W, C), float('nan'), device=DEV)
    plan._conv(pc, xin, None, N, H, W, y32, res=rn.to(DEV), in_fmt=1, **kw)
    torch.cuda.synchronize()
    if out_planes:
        stored_as_halves("planes in and out", val, nchw(y32.cpu()), parts)
        _, Ty = epilogue(Tz, z, es, et, 0, 0.0, r.double())
    check(f"PARTS {parts} planes in C{C} {N}x{H}x{W} [{kind}]", nchw(y32.cpu()), y, Ty)
    if zero:
        exact_channel("planes in", y32.cpu()[..., c0], T_(et)[:, c0][:, None, None] + rn[..., c0])


@pytest.mark.parametrize("parts", [2, 1])
@pytest.mark.parametrize("C,N,H,W,kind", [(64, 1, 64, 128, 'signed'), (32, 2, 37, 70, 'pos'), (128, 1, 23, 45, 'signed'), (64, 45, 30, 27, 'pos')])
def test_stride2_planes_in_planes4_out_second_output(parts, C, N, H, W, kind):
    """The stride-2 layer of the data flow: planes in, planes of 4 channels out, the second output SiLU(value) stored as halves."""
    from yond_public_amd.engine import _PackedConv
    Co = 2 * C
    rng, x, w, _, b = operands(9 + parts, C, Co, N, H, W, kind, H == 37, False)
    xin = to_planes(nhwc(T_(x)), parts)
    a64, _ = decode_planes(xin, N, C, H, W, parts)
    w = scale_to(w, F.conv2d(a64, T_(w).double(), stride=2, padding=1))
    z = F.conv2d(a64, T_(w).double(), stride=2, padding=1)
    Tz = M.threshold_conv(a64, T_(w), z, 2, parts)
    y, Ty = epilogue(Tz, z, None, b, 0, 0.0, None)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    plan = plan_with_status()
    pc = _PackedConv(plan.dev, T_(w), T_(b), 3, 2, [C])
    algo = 'split' if parts == 2 else 'half'
    gp4 = torch.full((N * Co * Ho * Wo,), float('nan'), device=DEV)
    second = plan._new_sp('second', N, Ho, Wo, Co, parts)
    plan._conv(pc, xin, None, N, H, W, gp4, algo=algo, in_fmt=1, out_fmt=2, dst2=second)
    torch.cuda.synchronize()
    assert int(plan.status[0]) == 0
    got = nchw(from_p4(gp4, N, Ho, Wo, Co))
    check(f"PARTS {parts} s2 planes -> planes of 4 C{C} {N}x{H}x{W} [{kind}]", got, y, Ty)
    val, pads = decode_planes(second, N, Co, Ho, Wo, parts)
    assert not pads.view(torch.int16).any()
    # the second output is SiLU of the float32 value the first output holds: 1.1-Lipschitz, the SiLU's own 2^-21, then the halves
    s = F.silu(y)
    Ts = 1.1 * Ty + 2.0 ** -21 * s.abs() + (2.0 ** -22 * s.abs() + 2.0 ** -36 if parts == 2 else 2.0 ** -11 * s.abs() + 2.0 ** -25)
    check(f"PARTS {parts} s2 second output C{C} [{kind}]", val, s, Ts)
    if H == 37:
        c0 = Co - 2
        exact_channel("s2 planes -> planes of 4", got[:, c0], T_(b)[c0].reshape(1, 1, 1))
        v0 = val[:, c0].reshape(-1)
        assert bool((v0 == v0[0]).all())                            # SiLU(bias) as halves: one value


def dec_eval(cur, skip, wf):
    """The decoder GEMM (ConvTranspose2d 2x2 over [cur | skip at the sub-position]) on float64 [N][h][w][2c], [N][2h][2w][c], [3c][c][2][2]."""
    c = wf.shape[1]
    N, h, w, _ = cur.shape
    r = torch.einsum('nyxi,iojk->nyjxko', cur, wf[:2 * c]).reshape(N, 2 * h, 2 * w, c)
    return r + torch.einsum('nyjxki,iojk->nyjxko', skip.reshape(N, h, 2, w, 2, c), wf[2 * c:]).reshape(N, 2 * h, 2 * w, c)


def dec_threshold(cur, skip, wf, ref, parts):
    a, s, w = cur.abs(), skip.abs(), wf.abs()
    sub = lambda t: ((t > 0) & (t < M.SUB)).double()
    Q = dec_eval(a * a, s * s, w * w).sqrt()
    floor = M.floor_unit(parts) * (dec_eval(sub(a), sub(s), w) + dec_eval(a, s, sub(w)))
    e, _ = M.rel_eps(3 * wf.shape[1], parts)
    return e * (Q + ref.abs()) + floor


DECODER_CASES = [(64, 24, 32, 2, 'signed', True), (32, 19, 33, 2, 'pos', True), (128, 9, 35, 2, 'signed', True), (64, 13, 11, 45, 'pos', True)]


@pytest.mark.parametrize("parts,c,h,w,N,kind,planes", [(2,) + c for c in DECODER_CASES] + [(1,) + c for c in DECODER_CASES] +
                         [(2, 64, 9, 20, 2, 'big', False), (2, 32, 9, 20, 2, 'signed', False)])
def test_decoder_gemm_with_skip(parts, c, h, w, N, kind, planes):
    """K1: the decoder's pixel-shuffle GEMM over [cur | skip] -- 32-channel and 64-channel tiles, plain and folded -- from planes (output
    float32, planes of 4 and the second output) or from [N][H][W][C] tensors (split operands only: the h-only form exists inside the flow)."""
    from yond_public_amd.engine import _PackedConv
    rng = np.random.default_rng([13 + parts, c, h, w])
    cur = nhwc(T_(M.stress_acts(rng, (N, 2 * c, h, w), kind)))
    skip = nhwc(T_(M.stress_acts(rng, (N, c, 2 * h, 2 * w), kind)))
    zero = h in (19, 24) or not planes                              # (one case of every variant: 32- / 64-channel tiles, with the second output, plain tensors)
    if zero:
        cur[..., 3] = 0.0
        skip[..., 3] = 0.0
    wf = np.ascontiguousarray(M.stress_weights(rng, c, 3 * c, 2, zero_out=c - 2 if zero else None, fan_in=3 * c).transpose(1, 0, 2, 3))
    bf = (10.0 ** rng.uniform(-2, 2, c) * rng.choice([-1.0, 1.0], c)).astype(np.float32)
    plan = plan_with_status()
    algo = 'split' if parts == 2 else 'half'
    if planes:
        cin, sin = to_planes(cur, parts), to_planes(skip, parts)
        c64 = nhwc(decode_planes(cin, N, 2 * c, h, w, parts)[0])
        s64 = nhwc(decode_planes(sin, N, c, 2 * h, 2 * w, parts)[0])
        wf = scale_to(wf, dec_eval(c64, s64, T_(wf).double()))
    else:
        c64, s64 = cur.double(), skip.double()
    z = dec_eval(c64, s64, T_(wf).double())
    Tz = dec_threshold(c64, s64, T_(wf).double(), z, parts)
    y = z + T_(bf).double()
    Ty = Tz + 2.0 ** -24 * (z.abs() + y.abs())
    pc = _PackedConv(plan.dev, T_(wf), T_(bf), 1, 1, [2 * c, c], shuffle=True)
    got = torch.full((N, 2 * h, 2 * w, c), float('nan'), device=DEV)
    if not planes:
        plan._conv(pc, cur.to(DEV), skip.to(DEV), N, h, w, got, algo=algo)
        torch.cuda.synchronize()
        check(f"decoder GEMM c{c} {N}x{h}x{w} [{kind}]", got.cpu(), y, Ty, ch_axis=3)
        exact_channel("decoder GEMM", got.cpu()[..., c - 2], T_(bf)[c - 2].reshape(1, 1, 1))
        return
    plan._conv(pc, cin, sin, N, h, w, got, algo=algo, in_fmt=1)
    gp4 = torch.full((N * c * 4 * h * w,), float('nan'), device=DEV)
    second = None
    if c >= 64 and w > 16:
        second = plan._new_sp('second', N, 2 * h, 2 * w, c, parts)
    plan._conv(pc, cin, sin, N, h, w, gp4, algo=algo, in_fmt=1, out_fmt=2, dst2=second)
    torch.cuda.synchronize()
    assert int(plan.status[0]) == 0
    check(f"PARTS {parts} decoder GEMM from planes c{c} {N}x{h}x{w} [{kind}]", got.cpu(), y, Ty, ch_axis=3)
    check(f"PARTS {parts} decoder GEMM from planes -> planes of 4 c{c}", from_p4(gp4, N, 2 * h, 2 * w, c), y, Ty, ch_axis=3)
    if second is not None:
        val, pads = decode_planes(second, N, c, 2 * h, 2 * w, parts)
        assert not pads.view(torch.int16).any()
        s = F.silu(nchw(y))
        Ts = 1.1 * nchw(Ty) + 2.0 ** -21 * s.abs() + (2.0 ** -22 * s.abs() + 2.0 ** -36 if parts == 2 else 2.0 ** -11 * s.abs() + 2.0 ** -25)
        check(f"PARTS {parts} decoder GEMM second output c{c}", val, s, Ts)
        if zero:
            v0 = val[:, c - 2].reshape(-1)
            assert bool((v0 == v0[0]).all())
    if zero:
        exact_channel("decoder GEMM from planes", got.cpu()[..., c - 2], T_(bf)[c - 2].reshape(1, 1, 1))
        exact_channel("decoder GEMM from planes -> planes of 4", from_p4(gp4, N, 2 * h, 2 * w, c)[..., c - 2], T_(bf)[c - 2].reshape(1, 1, 1))


@pytest.mark.parametrize("P,cin,cout,kind", [(1024, 64, 64, 'signed'), (333, 256, 96, 'pos'), (515, 32, 32, 'big')])
def test_gemm_split_f32(P, cin, cout, kind):
    """yond_gemm_split_f32 (gemm_split.hip: weights staged in three parts, one accumulator carrying 2^11) as a 1x1 convolution; its
    weights must stay below 32, so the stress weights are scaled to max|w| = 30.  Both tile widths (64 and 32 output channels)."""
    from test_hip_train import _gemm_split
    rng = np.random.default_rng([17, P, cin])
    x = M.stress_acts(rng, (1, cin, P, 1), kind)[0, :, :, 0].T.copy()                    # [P][cin]
    w = M.stress_weights(rng, cout, cin, 1)[:, :, 0, 0]
    w = (w * np.float32(30.0 / np.abs(w).max())).astype(np.float32)
    if P == 333:                                                    # the zero variant: an input channel and an output channel's weights
        x[:, 3] = 0.0
        w[cout - 2] = 0.0
    b = (10.0 ** rng.uniform(-2, 2, cout)).astype(np.float32)
    ref = x.astype(np.float64) @ w.astype(np.float64).T
    T = M.threshold_gemm(x, w.T, ref)
    y64 = ref + b.astype(np.float64)
    T = T + 2.0 ** -24 * (np.abs(ref) + np.abs(y64))
    xd, wd, bd = T_(x).to(DEV), T_(w).to(DEV), T_(b).to(DEV)
    y = torch.full((P, cout), float('nan'), device=DEV)
    assert _gemm_split([(xd.data_ptr(), wd.data_ptr(), 1, 0, cin, cin, 1 << 30, cin)], P, cout, cout, cin, 0, 1 << 30, bd, y, cout) == 0
    check(f"gemm_split {P}x{cin}->{cout} [{kind}]", y.cpu(), y64, T, ch_axis=1)
    if P == 333:
        exact_channel("gemm_split", y.cpu()[:, cout - 2][None], T_(b)[cout - 2].reshape(1, 1))


@pytest.mark.parametrize("N,cin,cout,H,W", [(2, 32, 64, 16, 32), (1, 64, 32, 13, 21)])
def test_wgrad_split_small_gradients(N, cin, cout, H, W):
    """yond_conv_wgrad_split_f32 (wgrad_split.hip: dy staged in three parts, pixel axis = K) with gradients spread over 10^4 below 1:
    most dy lie below fp16's normal range, where the P part must stay 2^11 h.  dw[tap][co][ci] against float64, per element."""
    from yond_public_amd import _lib as L
    lib = L.load()
    rng = np.random.default_rng([19, cin, H])
    x = M.stress_acts(rng, (N, cin, H, W), 'signed')
    dy = M.stress_acts(rng, (N, cout, H, W), 'signed') * np.float32(1e-2)
    xt, dyt = T_(x).double().requires_grad_(False), T_(dy).double()
    w = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(xt, w, padding=1).backward(dyt)
    ref = w.grad                                                    # [co][ci][3][3]
    # dw[co][ci][tap] = sum over pixels of dy[p][co] x[p + tap][ci]: the bound of a product sum with K = N H W
    sq = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(xt * xt, sq, padding=1).backward(dyt * dyt)
    sub = lambda t: ((t.abs() > 0) & (t.abs() < M.SUB)).double()
    f1 = torch.zeros_like(ref).requires_grad_(True)
    F.conv2d(sub(xt), f1, padding=1).backward(dyt.abs())
    f2 = torch.zeros_like(ref).requires_grad_(True)
    F.conv2d(xt.abs(), f2, padding=1).backward(sub(dyt))
    e, _ = M.rel_eps(N * H * W)
    T = e * (sq.grad.sqrt() + ref.abs()) + 2.0 ** -36 * (f1.grad + f2.grad)
    xd = nhwc(T_(x)).to(DEV)
    dyd = nhwc(T_(dy)).to(DEV)
    need = int(lib.yond_conv_wgrad_split_ws_bytes(N, H, W, cin, cout))
    ws = torch.zeros(need // 4, device=DEV)
    dw = torch.full((9, cout, cin), float('nan'), device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    L.check(lib.yond_conv_wgrad_split_f32(L.ptr(xd), L.ptr(dyd), N, H, W, cin, cout, L.ptr(dw), 0, L.ptr(ws), need, L.ptr(status), L.stream()), "wgrad_split")
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    got = dw.cpu().double().permute(1, 2, 0).reshape(cout, cin, 3, 3)
    check(f"wgrad_split N{N} {cin}->{cout} {H}x{W}", got, ref, T, ch_axis=0)
