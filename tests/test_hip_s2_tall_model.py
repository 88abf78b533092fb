"""GPU: the stride-2 layer on 8-row tiles (csrc/conv_s2_tall.hip, descriptor algo 7) against a float64 MODEL, not against the template: an
error the two kernels share -- the packed-weight layout, the n * Cout index of the per-image vectors -- passes every bit-for-bit test of
tests/test_hip_s2_tall*.py.  Reference: F.conv2d in float64 on the values decoded from the input planes; every output element against its
own bound, |got - ref| <= 4 T (tests/split_model.py), the second output against 1.1 T_y + 2^-21 |s| + 2^-22 |s| + 2^-36 (SiLU of the first
output's float32 value, stored as halves).  Operands as in tests/test_hip_s2_tall.py: stress activations with values planted at fp16's
subnormal boundary, heavy-tailed weights, scaled by one factor so that the outputs stay in fp16's range (the status word must stay 0).
Input 17 x 65 and 18 x 66, output 9 x 33: two row tiles and two column bands, ONE valid row in the second row tile and ONE valid pixel in
the second band; input row H and column W outside the frame (odd sizes) or the last real ones (even sizes).  Every case with the bias alone,
a per-image scale + shift (ebatch 1: a wrong image index shows) and the bias with a LeakyReLU, in both tile orders; one output channel has
zero weights and must hold the bias path bit for bit.  Both instantiations of both forms are launched, the two the engine does not use too.
Then: every tensor of a launch in the MIDDLE of a NaN-filled allocation (a stray read becomes a NaN in the output, a stray store changes
a fence), and the LDS room of the per-image vectors at exactly its limit (6 images x 256 channels) and one image past it, where the engine
keeps the template.  Every launch asserts its tag: /tall, or none for the fall-back."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import split_model as M
from test_hip_conv import DEV, bare_plan, from_p4, nchw, nhwc, sp_decode, to_sp
from test_hip_s2_tall import TAG, T_, run_pair, sp_floats
from test_hip_split_stress import check, epilogue, scale_to

pytestmark = pytest.mark.gpu

SIZES = [(17, 65), (18, 66)]
FENCE = 1 << 14                       # floats in front of and behind a tensor: the views stay 16-byte aligned
NAN_BITS = int(torch.tensor(float('nan')).view(torch.int32))


def plant():
    """fp16's subnormal boundary: the smallest normal number, its neighbours on both sides, the smallest subnormal, with both signs."""
    edge = np.float32(2.0 ** -14)
    return torch.tensor([edge, -edge, edge * (1 - 2.0 ** -11), edge * (1 + 2.0 ** -10), 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, 0.0])


def fenced(t):
    """A device tensor as the middle of a NaN-filled allocation: (view of t's shape, whole allocation)."""
    n = t.numel()
    big = torch.full((n + 2 * FENCE,), float('nan'), device=DEV)
    big[FENCE:FENCE + n] = t.reshape(-1).to(DEV)
    return big[FENCE:FENCE + n].view(t.shape), big


def fences_intact(big):
    b = big.view(torch.int32)
    return bool((b[:FENCE] == NAN_BITS).all()) and bool((b[-FENCE:] == NAN_BITS).all())


def films(rng, N, cout, bf):
    """(name, launch arguments, (es, et) of the model, post, slope) of the three epilogues."""
    es, et = M.stress_film(rng, N, cout)
    return [("bias", {}, (None, bf), 0, 0.0),
            ("scale + shift", dict(escale=T_(es).to(DEV), eshift=T_(et).to(DEV), ebatch=1), (es, et), 0, 0.0),
            ("bias + LeakyReLU", dict(post_act=2, slope=0.2), (None, bf), 2, 0.2)]


def second_bound(y, Ty):
    """SiLU of the float32 value the first output holds: 1.1-Lipschitz, the SiLU's own 2^-21, then the two halves."""
    s = F.silu(y)
    return s, 1.1 * Ty + 2.0 ** -21 * s.abs() + 2.0 ** -22 * s.abs() + 2.0 ** -36


def bias_path(es_et, post, slope, N, c0):
    """The float32 value of an output channel with zero weights, [N]: 0 * scale + shift, then the LeakyReLU as the kernel forms it."""
    es, et = es_et
    v = T_(et)[:, c0] if et.ndim == 2 else T_(et)[c0].expand(N)
    if post == 2:
        v = torch.where(v > 0, v, v * torch.tensor(slope, dtype=torch.float32))
    return v


def model(rng, cin, cout, N, H, W, kind='signed', zero=True, plant_edge=True):
    """Operands and their float64 twin: x in split planes, the values decoded from them, weights with an all-zero output channel."""
    x = nhwc(T_(M.stress_acts(rng, (N, cin, H, W), kind)))
    if plant_edge:
        x[..., 0:8] = plant()
    xin = to_sp(x)
    a64, _ = sp_decode(xin, N, cin, H, W)
    if kind == 'tame':
        wf = (rng.standard_normal((cout, cin, 3, 3)) / (3 * cin ** 0.5)).astype(np.float32)
        if zero:
            wf[cout - 2] = 0.0
    else:
        wf = M.stress_weights(rng, cout, cin, 3, zero_out=cout - 2 if zero else None)
    return xin, a64, wf


def reference(a64, wf):
    """(z, T_z) of the layer without its epilogue: computed once per case, shared by its launches."""
    z = F.conv2d(a64, T_(wf).double(), stride=2, padding=1)
    return z, M.threshold_conv(a64, T_(wf), z, stride=2, parts=2)


def verify(name, got, got2, ref, es_et, post, slope, N, cout, ho, wo, zero=True):
    """dst (planes of 4) and the second output (split planes or None) of one launch against the float64 model.  Returns (y, Ty) NCHW."""
    z, Tz = ref
    y, Ty = epilogue(Tz, z, es_et[0], es_et[1], post, slope, None)
    val = nchw(from_p4(got, N, ho, wo, cout))
    assert bool(torch.isfinite(val).all()), name
    check(name, val, y, Ty)
    c0 = cout - 2
    if zero:
        want = bias_path(es_et, post, slope, N, c0)[:, None, None].expand(N, ho, wo)
        assert torch.equal(val[:, c0].view(torch.int32), want.contiguous().view(torch.int32)), (name, "the zero-weight channel")
    if got2 is not None:
        v2, pads = sp_decode(got2, N, cout, ho, wo)
        assert not pads.view(torch.int16).any(), (name, "pad units of the second output")
        s, Ts = second_bound(y, Ty)
        check(name + ", second output", v2, s, Ts)
        if zero:
            flat = v2[:, c0].reshape(N, -1)
            assert bool((flat == flat[:, :1]).all()), (name, "SiLU(bias path) as halves: one value per image")
    return y, Ty


def status_plan():
    plan = bare_plan()
    plan.status, plan.status_slot = torch.zeros(4, dtype=torch.int32, device=DEV), 0
    return plan


def scaled(wf, a64, film_list):
    """One factor on the weights: max|output| ~ 3e4 over every epilogue of the case (the shift is not scaled; it stays below 100)."""
    z0 = F.conv2d(a64, T_(wf).double(), stride=2, padding=1)
    lin = z0.abs()
    for _, _, (es, _), _, _ in film_list:
        if es is not None:
            lin = torch.maximum(lin, (z0 * T_(es).double()[:, :, None, None]).abs())
    return scale_to(wf, lin)


# (Cin, Cout, second output, images): the four layers as the engine launches them, then the two exported instantiations it does not use today
CASES = [(32, 64, False, (1, 2)), (64, 128, False, (1, 2)), (128, 256, True, (1, 2)), (256, 512, True, (1,)), (32, 64, True, (2,)), (64, 128, True, (2,))]


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("cc", CASES, ids=lambda c: f"{c[0]}to{c[1]}{'_d2' if c[2] else ''}")
def test_s2_tall_against_float64(cc, hw):
    from yond_public_amd.engine import _PackedConv
    (cin, cout, d2, images), (H, W) = cc, hw
    ho, wo = (H + 1) // 2, (W + 1) // 2
    assert (ho, wo) == (9, 33)
    for N in images:
        rng = np.random.default_rng([43, cin, cout, int(d2), N, H])
        xin, a64, wf = model(rng, cin, cout, N, H, W)
        bf = (10.0 ** rng.uniform(-2, 2, cout) * rng.choice([-1.0, 1.0], cout)).astype(np.float32)
        fl = films(rng, N, cout, bf)
        wf = scaled(wf, a64, fl)
        ref = reference(a64, wf)
        plan = status_plan()
        pc = _PackedConv(plan.dev, T_(wf), T_(bf), 3, 2, [cin])
        for fname, kw, es_et, post, slope in fl:
            for order in (0, 1):
                out = run_pair(plan, pc, xin, N, H, W, cout, d2, order, **kw)         # (asserts the tags: the template, then /tall)
                torch.cuda.synchronize()
                st = plan.status.cpu()
                name = f"algo 7 c{cin}->{cout}{' +second' if d2 else ''} N{N} {H}x{W} film={fname} order={order}"
                assert int(st[0]) == 0 and int(st[1]) == 0, (name, st)
                verify(name, out[True][0], out[True][1], ref, es_et, post, slope, N, cout, ho, wo)


# ---- NaN fences round every tensor ----------------------------------------------------------------------------------------------------

def launch_tall(plan, pc, xin, N, H, W, dst, dst2, order, tall_tag=True, **kw):
    plan._tile_order = 1 - order
    plan.prof = []
    plan._conv(pc, xin, None, N, H, W, dst, algo='split', in_fmt=1, out_fmt=2, dst2=dst2, s2_tall=True, **kw)
    tags, plan.prof = [pr[0] for pr in plan.prof], None
    assert tags == [TAG + ("/tall" if tall_tag else "")], tags


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("cin,cout,d2", [(32, 64, False), (128, 256, True)], ids=["one_image_form", "two_image_form_d2"])
def test_s2_tall_inside_nan_fences(cin, cout, d2, hw):
    """Tame data; the input planes, dst and the second output each the middle of a NaN-filled allocation.  The two-image form sends the pad units
    of its LDS rows and the units behind the four planes to the plane's zero unit, the one-image form its items past the tile: a unit read
    outside the planes is a NaN in an accumulator, a store outside dst changes a fence."""
    from yond_public_amd.engine import _PackedConv
    H, W = hw
    N, ho, wo = 2, (H + 1) // 2, (W + 1) // 2
    rng = np.random.default_rng([47, cin, H])
    xin, a64, wf = model(rng, cin, cout, N, H, W, kind='tame', plant_edge=False)
    bf = rng.standard_normal(cout).astype(np.float32)
    plan = status_plan()
    pc = _PackedConv(plan.dev, T_(wf), T_(bf), 3, 2, [cin])
    xv, x_all = fenced(xin)
    ref = reference(a64, wf)
    for order in (0, 1):
        dv, d_all = fenced(torch.zeros(N * cout * ho * wo))
        sv, s_all = fenced(torch.zeros(sp_floats(N, cout, ho, wo))) if d2 else (None, None)
        launch_tall(plan, pc, xv, N, H, W, dv, sv, order)
        torch.cuda.synchronize()
        name = f"algo 7 in NaN fences c{cin}->{cout} {H}x{W} order={order}"
        assert int(plan.status[0]) == 0, name
        assert fences_intact(d_all) and fences_intact(x_all) and (not d2 or fences_intact(s_all)), name
        assert torch.equal(xv.view(torch.int32), xin.view(torch.int32)), name
        verify(name, dv, sv, ref, (None, bf), 0, 0.0, N, cout, ho, wo)


# ---- the LDS room of the per-image vectors ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,tall", [(6, True), (7, False)], ids=["at_the_limit", "one_past_it"])
def test_s2_tall_vector_room(N, tall):
    """64 -> 256 channels, input 2 x 34 (output 1 x 17), a scale + shift pair per image: 6 x 256 = 1536 floats fill the kernel's room exactly --
    the last image's last channel reads the last float of each vector's LDS range -- and 7 images do not fit: the engine keeps the template."""
    from yond_public_amd.engine import _PackedConv
    cin, cout, H, W = 64, 256, 2, 34
    ho, wo = 1, 17
    rng = np.random.default_rng([53, N])
    xin, a64, wf = model(rng, cin, cout, N, H, W)
    es, et = M.stress_film(rng, N, cout)
    plan = status_plan()
    pc = _PackedConv(plan.dev, T_(wf), None, 3, 2, [cin])
    kw = dict(escale=T_(es).to(DEV), eshift=T_(et).to(DEV), ebatch=1)
    ref = reference(a64, wf)
    for order in (0, 1):
        dv, d_all = fenced(torch.zeros(N * cout * ho * wo))
        launch_tall(plan, pc, xin, N, H, W, dv, None, order, tall_tag=tall, **kw)
        torch.cuda.synchronize()
        name = f"algo 7 vector room N{N} ({'/tall' if tall else 'template'}) order={order}"
        assert int(plan.status[0]) == 0 and fences_intact(d_all), name
        y, Ty = verify(name, dv, None, ref, (es, et), 0, 0.0, N, cout, ho, wo)
        val = nchw(from_p4(dv, N, ho, wo, cout))
        check(name + ", last image, last channel", val[N - 1:, cout - 1:], y[N - 1:, cout - 1:], Ty[N - 1:, cout - 1:])
        # ... whose zero-weight neighbour holds exactly the last image's shift
        assert torch.equal(val[N - 1, cout - 2], T_(et)[N - 1, cout - 2].expand(ho, wo)), name
