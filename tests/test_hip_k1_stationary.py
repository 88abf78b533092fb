"""GPU: the decoder GEMM with stationary weights (csrc/gemm_k1_stationary.hip, descriptor algo 6) against the K1 form of the split-operand
template (conv_split_kernel.h, algo 3) -- the same descriptor, the same packed weights, the same split-plane inputs -- BIT FOR BIT: per
accumulator the new kernel issues the template's MFMA sequence and its epilogue is the template's, so nothing may differ.
Shapes (low resolution H x W): a single pixel (every other lane on the zero unit), one pixel into the second segment, ragged edges, exact
multiples of the segment, one past a multiple; one and two images; both tile orders; the bias alone (what the engine passes), a per-image
scale + shift, and the bias with a LeakyReLU behind it.  Operands: stress activations (10^-4 .. 1, many below fp16's normal range) with values planted at fp16's subnormal boundary,
heavy-tailed weights, and a 16-channel chunk of the skip tensor that holds 6e4 everywhere behind all-zero weights.
Channels (low-resolution input, skip tensor): (64, 32) in the two-sub-positions form with the [N][H][W][C] store (level 1 -> 0), whose zero-weight
chunk re-reads the skip tensor's first 16 channels; (128, 64) and (256, 128) with the planes-of-4 store (levels 2 -> 1 and 3 -> 2).
Then one whole GuidedResUnet forward with the engine's per-level switch on and off, and the build's resource report."""
import numpy as np
import pytest
import torch

import split_model as M
from hip_common import ARCHS, make_net
from test_hip_conv import DEV, bare_plan, nhwc, to_sp

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 33), (9, 31), (8, 64), (17, 65)]
CHANNELS = [(64, 32), (128, 64), (256, 128)]          # (C0, C1): low-resolution input, skip tensor = channels of an output pixel


def T_(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("cc", CHANNELS)
def test_stationary_gemm_equals_template_bit_for_bit(cc, hw):
    from yond_public_amd.engine import _PackedConv, _PackedUpSub2
    (c0, c), (h, w) = cc, hw
    assert c0 == 2 * c
    rng = np.random.default_rng([29, c, h, w])
    wf = M.stress_weights(rng, c, 3 * c, 2, fan_in=3 * c).transpose(1, 0, 2, 3).copy()        # [2c cur + c skip][c][2][2]
    wf[2 * c + 16:2 * c + 32] = 0.0                   # a chunk of the skip tensor with zero weights ...
    bf = (10.0 ** rng.uniform(-2, 2, c) * rng.choice([-1.0, 1.0], c)).astype(np.float32)
    plan = bare_plan()
    plan.status, plan.status_slot = torch.zeros(4, dtype=torch.int32, device=DEV), 0
    sub2 = c == 32                                    # the two-sub-positions form, [N][H][W][C] out; else shuffle 1, planes of 4 out
    pc = _PackedUpSub2(plan.dev, T_(wf), T_(bf), c) if sub2 else _PackedConv(plan.dev, T_(wf), T_(bf), 1, 1, [2 * c, c], shuffle=True)
    assert not sub2 or pc.ok
    edge = np.float32(2.0 ** -14)
    for N in (1, 2):
        cur = nhwc(T_(M.stress_acts(rng, (N, 2 * c, h, w), 'signed')))
        skip = nhwc(T_(M.stress_acts(rng, (N, c, 2 * h, 2 * w), 'signed')))
        # fp16's subnormal boundary: the smallest normal number, its neighbours on both sides, the smallest subnormal, with both signs
        plant = torch.tensor([edge, -edge, edge * (1 - 2.0 ** -11), edge * (1 + 2.0 ** -10), 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, 0.0])
        cur[..., 0:8] = plant
        skip[:, 0, 0, c - 24:c - 16] = plant
        skip[..., 16:32] = 6.0e4                      # ... and large finite data
        if sub2:
            skip[..., 8:16] = 6.0e4                   # (the form's own zero-weight chunk reads channels 0 .. 15 again)
        cin, sin = to_sp(cur), to_sp(skip)
        es, et = M.stress_film(rng, N, c)
        for film, kw in (("bias", {}), ("scale + shift", dict(escale=T_(es).to(DEV), eshift=T_(et).to(DEV), ebatch=1)),
                         ("bias + LeakyReLU", dict(post_act=2, slope=0.2))):
            for order in (0, 1):
                out = {}
                for stationary in (False, True):
                    got = torch.full((N * c * 4 * h * w,), float('nan'), device=DEV)
                    plan._tile_order = 1 - order      # (the engine alternates the order from launch to launch)
                    plan.prof = []
                    plan._conv(pc, cin, sin, N, h, w, got, algo='split', in_fmt=1, out_fmt=0 if sub2 else 2, stationary=stationary, **kw)
                    tags, plan.prof = [pr[0] for pr in plan.prof], None
                    assert tags == ["conv_split_kernel<k1,64,2>" + ("/stationary" if stationary else "")], tags
                    out[stationary] = got
                torch.cuda.synchronize()
                name = f"c{c} N{N} {h}x{w} film={film} order={order}"
                assert bool(torch.isfinite(out[False]).all()), name
                assert torch.equal(bits(out[True]), bits(out[False])), (name, int((bits(out[True]) != bits(out[False])).sum()))
    assert int(plan.status[0]) == 0


def test_forward_with_and_without_stationary_levels():
    """One GuidedResUnet forward at a packed size of 64 x 96 with the engine's switch on for all three levels, and off:
    the outputs are bit-equal and so is the status word."""
    from yond_public_amd import engine as E
    net, _ = make_net(dict(ARCHS["gru32"]), 11)
    x = (torch.rand((1, 4, 64, 96), generator=torch.Generator().manual_seed(3)) * 0.9).to(DEV)
    t = torch.tensor(0.05).to(DEV)
    plan = net._get_plan(torch.device(DEV))
    assert plan._sp_flow(1, 64, 96)
    saved = E.K1_STATIONARY_LEVELS
    res = {}
    try:
        for levels in ((2, 1, 0), ()):
            E.K1_STATIONARY_LEVELS = levels
            plan.prof = []
            with torch.no_grad():
                y = net(x, t)
            torch.cuda.synchronize()
            res[levels] = (y.clone(), plan.status.clone(), [pr[0].endswith("/stationary") for pr in plan.prof])
    finally:
        E.K1_STATIONARY_LEVELS = saved
        plan.prof = None
    on = res[(2, 1, 0)]
    assert on[2].count(True) == 3 and res[()][2].count(True) == 0, (on[2], res[()][2])
    assert bool(torch.isfinite(res[()][0]).all())
    assert torch.equal(bits(on[0]), bits(res[()][0]))
    assert torch.equal(on[1], res[()][1])


def test_stationary_kernels_use_no_scratch():
    """The build's resource report (the one tests/test_build_report.py reads): no scratch, no spilled register in any instantiation."""
    from yond_public_amd import build as B
    full = B.resource_report()
    if not full:
        pytest.skip("a shipped library without its object directory or link-time report: nothing to check here")
    rep = [r for r in full if "gemm_k1_stationary_kernel" in r["name"]]
    assert len(rep) >= 3, rep
    bad = [r for r in rep if r.get("scratch", 0) or r.get("vgpr_spill", 0) or r.get("sgpr_spill", 0)]
    assert not bad, bad
