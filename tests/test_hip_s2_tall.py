"""GPU: the stride-2 layer on 8-row tiles, two output rows per wave, one input image in LDS (csrc/conv_s2_tall.hip, descriptor algo 7)
against the stride-2 form of the split-operand template (conv_split_kernel.h, algo 3) -- the same descriptor, the same packed weights, the
same split-plane input -- BIT FOR BIT: per accumulator the new kernel issues the template's MFMA sequence and its epilogue is the template's
epilogue_direct, so nothing may differ, neither in dst, nor in the second output, nor in the status word.
Output shapes Ho x Wo (input 2 Ho x 2 Wo): a single pixel, one pixel into the second 32-pixel column band, rows below / at / one past a
tile with ragged and exact columns, three row tiles with a ragged third band; one and two images; both tile orders; the bias alone (what the
engine passes), a per-image scale + shift, the bias with a LeakyReLU behind it.  Operands: stress activations (10^-4 .. 1, many below fp16's
normal range) with values planted at fp16's subnormal boundary, heavy-tailed weights.  Channels (32 -> 64), (64 -> 128) without the second
output, (128 -> 256), (256 -> 512) with it; one case of the latter kind stores a value whose SiLU exceeds 65504: both kernels raise the flag.
Then one whole GuidedResUnet forward with the engine's per-level switch full and empty, and the build's resource report."""
import numpy as np
import pytest
import torch

import split_model as M
from hip_common import ARCHS, make_net
from test_hip_conv import DEV, bare_plan, nhwc, to_sp

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 33), (7, 31), (8, 64), (9, 32), (17, 65)]
CHANNELS = [(32, 64, False), (64, 128, False), (128, 256, True), (256, 512, True)]     # (Cin, Cout, second output)
TAG = "conv_split_kernel<2,64,2>"


def T_(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def bits(t):
    return t.view(torch.int32)


def sp_floats(N, C, H, W):
    from yond_public_amd.engine import sp_plane_units
    return N * (C // 16) * 4 * sp_plane_units(H, W) * 4


def run_pair(plan, pc, xin, N, H, W, cout, d2, order, **kw):
    """The layer on the template (status slot 0) and on the new kernel (slot 1): {tall: (dst, dst2)}."""
    ho, wo = (H + 1) // 2, (W + 1) // 2
    out = {}
    for tall in (False, True):
        got = torch.full((N * cout * ho * wo,), float('nan'), device=DEV)
        got2 = torch.zeros(sp_floats(N, cout, ho, wo), device=DEV) if d2 else None      # (the zero pad is the caller's)
        plan._tile_order = 1 - order              # (the engine alternates the order from launch to launch)
        plan.status_slot = 1 if tall else 0
        plan.prof = []
        plan._conv(pc, xin, None, N, H, W, got, algo='split', in_fmt=1, out_fmt=2, dst2=got2, s2_tall=tall, **kw)
        tags, plan.prof = [pr[0] for pr in plan.prof], None
        assert tags == [TAG + ("/tall" if tall else "")], tags
        out[tall] = (got, got2)
    return out


@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("cc", CHANNELS)
def test_s2_tall_equals_template_bit_for_bit(cc, hw):
    from yond_public_amd.engine import _PackedConv
    (cin, cout, d2), (ho, wo) = cc, hw
    H, W = 2 * ho, 2 * wo
    rng = np.random.default_rng([31, cin, ho, wo])
    wf = M.stress_weights(rng, cout, cin, 3)
    bf = (10.0 ** rng.uniform(-2, 2, cout) * rng.choice([-1.0, 1.0], cout)).astype(np.float32)
    plan = bare_plan()
    plan.status = torch.zeros(4, dtype=torch.int32, device=DEV)
    pc = _PackedConv(plan.dev, T_(wf), T_(bf), 3, 2, [cin])
    edge = np.float32(2.0 ** -14)
    # fp16's subnormal boundary: the smallest normal number, its neighbours on both sides, the smallest subnormal, with both signs
    plant = torch.tensor([edge, -edge, edge * (1 - 2.0 ** -11), edge * (1 + 2.0 ** -10), 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, 0.0])
    for N in (1, 2):
        x = nhwc(T_(M.stress_acts(rng, (N, cin, H, W), 'signed')))
        x[..., 0:8] = plant
        xin = to_sp(x)
        es, et = M.stress_film(rng, N, cout)
        for film, kw in (("bias", {}), ("scale + shift", dict(escale=T_(es).to(DEV), eshift=T_(et).to(DEV), ebatch=1)),
                         ("bias + LeakyReLU", dict(post_act=2, slope=0.2))):
            for order in (0, 1):
                out = run_pair(plan, pc, xin, N, H, W, cout, d2, order, **kw)
                torch.cuda.synchronize()
                name = f"c{cin}->{cout} N{N} {ho}x{wo} film={film} order={order}"
                assert bool(torch.isfinite(out[False][0]).all()), name
                assert torch.equal(bits(out[True][0]), bits(out[False][0])), (name, int((bits(out[True][0]) != bits(out[False][0])).sum()))
                if d2:
                    assert torch.equal(bits(out[True][1]), bits(out[False][1])), (name, int((bits(out[True][1]) != bits(out[False][1])).sum()))
                    assert bool((bits(out[False][1]) != 0).any()), name
    st = plan.status.cpu()
    assert int(st[0]) == int(st[1]), st
    if not d2:
        assert int(st[0]) == 0, st                # (a consumer of finished planes raises nothing)


def test_s2_tall_raises_the_range_flag_where_the_template_does():
    """A second output whose SiLU exceeds 65504 (one channel's bias is 1e5): the same flag, the same bits -- the h half is +inf in both."""
    from yond_public_amd.engine import _PackedConv
    cin, cout, ho, wo, N = 128, 256, 9, 32, 1
    H, W = 2 * ho, 2 * wo
    rng = np.random.default_rng([37, cin, ho, wo])
    wf = M.stress_weights(rng, cout, cin, 3)
    wf *= np.float32(1.0 / max(1.0, np.abs(wf).max()))           # tame products: only the planted channel leaves the range
    bf = rng.uniform(-1, 1, cout).astype(np.float32)
    bf[37] = 1.0e5
    plan = bare_plan()
    plan.status = torch.zeros(4, dtype=torch.int32, device=DEV)
    pc = _PackedConv(plan.dev, T_(wf), T_(bf), 3, 2, [cin])
    xin = to_sp(nhwc(T_(M.stress_acts(rng, (N, cin, H, W), 'signed'))))
    out = run_pair(plan, pc, xin, N, H, W, cout, True, 0)
    torch.cuda.synchronize()
    st = plan.status.cpu()
    assert int(st[0]) & 1, st                     # YOND_STATUS_HALF_OVERFLOW
    assert int(st[0]) == int(st[1]), st
    assert torch.equal(bits(out[True][0]), bits(out[False][0]))
    assert torch.equal(bits(out[True][1]), bits(out[False][1]))


def test_forward_with_and_without_s2_tall_levels():
    """One GuidedResUnet forward at a packed size of 64 x 96 with the engine's switch on for all four levels, and off: four launches are
    tagged /tall (none when it is empty), the outputs are bit-equal and so is the status word."""
    from yond_public_amd import engine as E
    net, _ = make_net(dict(ARCHS["gru32"]), 11)
    x = (torch.rand((1, 4, 64, 96), generator=torch.Generator().manual_seed(3)) * 0.9).to(DEV)
    t = torch.tensor(0.05).to(DEV)
    plan = net._get_plan(torch.device(DEV))
    assert plan._sp_flow(1, 64, 96)
    saved = E.S2_TALL_LEVELS
    res = {}
    try:
        for levels in ((0, 1, 2, 3), ()):
            E.S2_TALL_LEVELS = levels
            plan.prof = []
            with torch.no_grad():
                y = net(x, t)
            torch.cuda.synchronize()
            res[levels] = (y.clone(), plan.status.clone(), [pr[0].endswith("/tall") for pr in plan.prof])
    finally:
        E.S2_TALL_LEVELS = saved
        plan.prof = None
    on = res[(0, 1, 2, 3)]
    assert on[2].count(True) == 4 and res[()][2].count(True) == 0, (on[2], res[()][2])
    assert bool(torch.isfinite(res[()][0]).all())
    assert torch.equal(bits(on[0]), bits(res[()][0]))
    assert torch.equal(on[1], res[()][1])


def test_s2_tall_kernels_use_no_scratch():
    """The build's resource report (the one tests/test_build_report.py reads): no scratch, no spilled register in either instantiation."""
    from yond_public_amd import build as B
    full = B.resource_report()
    if not full:
        pytest.skip("a shipped library without its object directory or link-time report: nothing to check here")
    rep = [r for r in full if "conv_s2_tall_kernel" in r["name"]]
    assert len(rep) >= 2, rep
    bad = [r for r in rep if r.get("scratch", 0) or r.get("vgpr_spill", 0) or r.get("sgpr_spill", 0)]
    assert not bad, bad
