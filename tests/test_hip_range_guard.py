"""The range guard of the half-precision operand paths at every site that raises it.

A kernel that stages or stores an fp32 value as fp16 halves ORs bit 0 into its status word when a value leaves fp16's range
(|a| > 65504) or is NaN; the host then repeats the forward on the fp32-input kernels.  The raising sites, from
`grep -nE "atomicOr[(].*(status|YOND_STATUS_)" yond_public_amd/csrc` (SITES below holds the same list for the CPU test that keeps it current):

  conv_split_kernel.h  one atomicOr at the kernel's end for three accumulation sites: the staged input (NHWC / planes of 4), the
                       split-plane or h-only-plane store (PRODUCER side: the consumer reads finished halves by LDS-DMA and
                       cannot see the value), the second output SiLU(value) (dst2, producer side)
  conv_s2_tall.hip     the stride-2 layer on 8-row tiles (descriptor algo 7), both forms: its second output SiLU(value) (dst2, producer side); the
                       pointer is parked in a vector register under another name, the flag constant names the site
  conv.hip             the generic kernel's half-precision modes (fp16 fragments, algo 2; split operands for 1x1 layers, algo 5)
  gemm_split.hip       two words: word 0 an x operand, word 1 a weight with |w| >= 32
  wgrad_split.hip      a staged 2^11 dy part: |dy| >= 31.9
  conv_split.hip       the two device-side weight packers of the training step: a weight beyond 65504 (the single-layer packer is probed
                       below; the batched one applies the same per-element test and is launched by the training-step tests, its flag
                       is not probed on its own)

Kernel level: ONE element of a well-scaled tensor replaced, at the first pixel / first channel, the last valid pixel of a ragged
tile / last real channel, and an interior position: 65000 leaves the word at 0 and the output within the split-operand bound
(tests/split_model.py); 7.0e4, +inf and NaN set the bit.  False positives: ragged tiles and zero-padded channels inside a larger
NaN-filled allocation must neither raise the flag nor touch the canary.  The 8-row stride-2 kernel's site: ONE output element at 6.0e4 / 1.0e5
at the first pixel, the last valid pixel of the ragged tiles, lane 31 of a full tile and an interior pixel, first and last channel, beside the
template in a second status slot; and across the tile walk of its persistent workgroups.  Network level: one layer regained by 1e6 and its
consumer by 1e-6 at five depths of three networks on both precisions.
Known and left as it is: in the epilogues that store halves (epilogue_sp, epilogue_direct, the 8-row kernel's) the masked lanes of a partial tile add
the finite values they formed from real input rows to the guard's maximum, so a crafted input can raise the flag with no stored value out of range --
the guard is conservative there, the repeated fp32 forward is still correct."""
import os
import re
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import split_model as M

gpu = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# file -> number of `atomicOr(<...>status...` / `atomicOr(<...>YOND_STATUS_...` statements the table above accounts for
SITES = {"conv_split_kernel.h": 1, "conv_s2_tall.hip": 1, "conv.hip": 1, "gemm_split.hip": 2, "wgrad_split.hip": 1, "conv_split.hip": 2}


def test_every_raising_site_is_in_the_table():
    """CPU: a csrc/ file that gains (or loses) an atomicOr on a status word must be added to the table and get a test."""
    csrc = os.path.join(ROOT, "yond_public_amd", "csrc")
    found = {}
    for name in sorted(os.listdir(csrc)):
        if not name.endswith(('.hip', '.h')):
            continue
        with open(os.path.join(csrc, name)) as f:
            # (one match per atomicOr whose statement names a status pointer or a status flag, whatever the pointer is called)
            n = len(re.findall(r"atomicOr\([^;]*?(?:status|YOND_STATUS_)", f.read()))
        if n:
            found[name] = n
    assert found == SITES, found


def T_(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def status_plan():
    from test_hip_conv import bare_plan
    plan = bare_plan()
    plan.status, plan.status_slot = torch.zeros(4, dtype=torch.int32, device=DEV), 0
    return plan


def word(plan):
    torch.cuda.synchronize()
    v = int(plan.status[0])
    plan.status.zero_()
    return v


def positions(N, H, W, C):
    """(first pixel, first channel), (last pixel, last real channel), an interior position of an [N][H][W][.] tensor."""
    return [(0, 0, 0, 0), (N - 1, H - 1, W - 1, C - 1), (N // 2, H // 2, W // 2, C // 2)]


BAD = (7.0e4, float('inf'), float('nan'))


def tame(seed, N, C, H, W, Co, k=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, C, generator=g)
    w = torch.randn(Co, C, k, k, generator=g) / (k * C ** 0.5)
    b = torch.randn(Co, generator=g)
    return g, x, w, b


# form, C real, C padded, Co, N, H, W, stride, algo, parts of the bound
STAGING = [
    ("s1 32 ragged", 32, 32, 32, 1, 9, 33, 1, 'split', 2),
    ("s1 64 ragged", 64, 64, 64, 2, 17, 40, 1, 'split', 2),
    ("s1 128 aligned", 128, 128, 128, 1, 8, 32, 1, 'split', 2),
    ("s1 folded ragged", 64, 64, 64, 5, 13, 11, 1, 'split', 2),
    ("s1 nf-8 zero padding", 8, 32, 32, 1, 17, 40, 1, 'split', 2),
    ("s2 ragged", 32, 32, 64, 1, 19, 35, 2, 'split', 2),
    ("s2 folded ragged", 64, 64, 128, 70, 11, 13, 2, 'split', 2),
    ("h-only s1 ragged", 64, 64, 64, 1, 17, 40, 1, 'half', 1),
    ("h-only 128-channel tiles", 64, 64, 128, 1, 13, 33, 1, 'half', 1),
    ("h-only s2 ragged", 32, 32, 64, 1, 19, 35, 2, 'half', 1),
    ("generic fp16 fragments 3x3", 64, 64, 64, 1, 17, 40, 1, 'fp16', 1),
]


@gpu
@pytest.mark.parametrize("case", STAGING, ids=[c[0].replace(' ', '_') for c in STAGING])
def test_staged_input_single_element(case):
    """The input-staging site of every 3x3 form (and conv.hip's fp16 mode): one element of a tame [N][H][W][C] tensor."""
    from yond_public_amd.engine import _PackedConv
    name, C, Cp, Co, N, H, W, stride, algo, parts = case
    g, x, w, b = tame(len(name) + H, N, C, H, W, Co)
    plan = status_plan()
    pc = _PackedConv(plan.dev, w, b, 3, stride, [C])
    Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if stride == 2 else (H, W)
    pre = int(stride == 1)                                          # (the stride-2 forms have no staged SiLU)

    def launch(xc):
        xp = torch.zeros(N, H, W, Cp)
        xp[..., :C] = xc
        dst = torch.full((N, Ho, Wo, pc.coutp), float('nan'), device=DEV)
        plan._conv(pc, xp.to(DEV), None, N, H, W, dst, algo=algo, pre_act=pre)
        return word(plan), dst.cpu()

    assert launch(x)[0] == 0
    for pos in positions(N, H, W, C):
        xc = x.clone()
        xc[pos] = 65000.0
        st, got = launch(xc)
        assert st == 0, (name, pos)
        a64 = xc.permute(0, 3, 1, 2).double()
        a64 = F.silu(a64) if pre else a64
        z = F.conv2d(a64, w.double(), stride=stride, padding=1)
        Tz = M.threshold_conv(a64, w, z, stride, parts, pre_silu=bool(pre))
        y, Ty = M.through_epilogue(Tz, z, None, b.double()[None, :, None, None])
        r = M.ratio_report(f"guard: {name}, 65000 at {pos}", got.permute(0, 3, 1, 2)[:, :Co], y, Ty)
        assert r.max() <= M.FACTOR
        assert float(got[..., Co:].abs().max() if pc.coutp > Co else 0.0) == 0.0
        for bad in BAD:
            xc[pos] = bad
            assert launch(xc)[0] & 1, (name, pos, bad)


@gpu
@pytest.mark.parametrize("algo,parts", [('split', 2), ('half', 1)])
@pytest.mark.parametrize("C,Cp,N,H,W", [(64, 64, 2, 17, 40), (8, 32, 1, 9, 33), (32, 32, 3, 13, 11)])
def test_no_false_positive_inside_a_nan_filled_allocation(algo, parts, C, Cp, N, H, W):
    """Ragged tiles, folded tiles and an nf-8 layer's zero channel padding, input and output tensors the front part of larger
    allocations filled with NaN: whatever a partial tile's masked lanes read or accumulate reaches neither the flag nor the canary."""
    from yond_public_amd.engine import _PackedConv
    g, x, w, b = tame(C + H, N, C, H, W, C)
    plan = status_plan()
    pc = _PackedConv(plan.dev, w, b, 3, 1, [C])
    n_in, n_out, tail = N * H * W * Cp, N * H * W * pc.coutp, 1 << 16
    big_in = torch.full((n_in + tail,), float('nan'), device=DEV)
    big_out = torch.full((n_out + tail,), float('nan'), device=DEV)
    xp = torch.zeros(N, H, W, Cp)
    xp[..., :C] = x
    big_in[:n_in] = xp.reshape(-1).to(DEV)
    plan._conv(pc, big_in[:n_in].view(N, H, W, Cp), None, N, H, W, big_out[:n_out].view(N, H, W, pc.coutp), algo=algo)
    assert word(plan) == 0
    assert bool(torch.isnan(big_out[n_out:]).all()) and bool(torch.isnan(big_in[n_in:]).all())
    got = big_out[:n_out].view(N, H, W, pc.coutp).cpu()
    a64 = x.permute(0, 3, 1, 2).double()
    z = F.conv2d(a64, w.double(), padding=1)
    y, Ty = M.through_epilogue(M.threshold_conv(a64, w, z, 1, parts), z, None, b.double()[None, :, None, None])
    r = M.ratio_report(f"guard: no false positive {algo} C{C} {N}x{H}x{W}", got.permute(0, 3, 1, 2)[:, :C], y, Ty)
    assert r.max() <= M.FACTOR
    assert float(got[..., C:].abs().max() if pc.coutp > C else 0.0) == 0.0


def in_canary(t, tail=1 << 14):
    """A flat float32 device buffer as the front part of a NaN-filled allocation: (view, whole allocation, length)."""
    n = t.numel()
    big = torch.full((n + tail,), float('nan'), device=DEV)
    big[:n] = t.reshape(-1)
    return big[:n], big, n


@gpu
@pytest.mark.parametrize("parts", [2, 1])
@pytest.mark.parametrize("C,N,H,W", [(64, 2, 17, 40), (32, 1, 9, 33), (64, 3, 13, 11)])
def test_no_false_positive_in_the_plane_flow_inside_nan_filled_allocations(parts, C, N, H, W):
    """The PRODUCER-side sites on ragged and folded tiles, every tensor the front part of a NaN-filled allocation: conv2 of a block (planes in
    by LDS-DMA, residual in planes of 4, planes out) and the stride-2 layer (planes in, planes of 4 out, the second output as halves).  Their
    masked lanes form values too (and the guard's maximum now sees a NaN): none may reach the flag, the canaries, or the planes' zero pads."""
    from test_hip_conv import hp_decode, sp_decode, to_hp, to_p4, to_sp
    from yond_public_amd.engine import _PackedConv
    g, x, w, b = tame(C + W, N, C, H, W, C)
    r = torch.randn(N, H, W, C, generator=g)
    algo = 'split' if parts == 2 else 'half'
    planes = to_sp if parts == 2 else to_hp
    decode = (lambda t, c, hh, ww: sp_decode(t, N, c, hh, ww)) if parts == 2 else (lambda t, c, hh, ww: hp_decode(t, N, c, hh, ww))
    plan = status_plan()
    ones = torch.ones(N, C, device=DEV)
    shift = b.to(DEV)[None].expand(N, C).contiguous()
    xin, xin_all, n_x = in_canary(planes(x))
    res, res_all, n_r = in_canary(to_p4(r))
    out, out_all, n_o = in_canary(torch.zeros_like(plan._new_sp('o', N, H, W, C, parts)))
    pc = _PackedConv(plan.dev, w, None, 3, 1, [C])
    plan._conv(pc, xin, None, N, H, W, out, res=res, in_fmt=1, out_fmt=1, res_fmt=2, escale=ones, eshift=shift, ebatch=1, algo=algo)
    assert word(plan) == 0
    for whole, n in ((xin_all, n_x), (res_all, n_r), (out_all, n_o)):
        assert bool(torch.isnan(whole[n:]).all())
    val, pads = decode(out, C, H, W)
    assert bool(torch.isfinite(val.double()).all()) and not pads.view(torch.int16).any()
    # the stride-2 layer with its second output
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    w2 = torch.randn(2 * C, C, 3, 3, generator=g) / (3 * C ** 0.5)
    b2 = torch.randn(2 * C, generator=g)
    pc2 = _PackedConv(plan.dev, w2, b2, 3, 2, [C])
    gp4, gp4_all, n_g = in_canary(torch.zeros(N * 2 * C * Ho * Wo, device=DEV))
    sec, sec_all, n_s = in_canary(torch.zeros_like(plan._new_sp('second', N, Ho, Wo, 2 * C, parts)))
    plan._conv(pc2, xin, None, N, H, W, gp4, algo=algo, in_fmt=1, out_fmt=2, dst2=sec)
    assert word(plan) == 0
    for whole, n in ((xin_all, n_x), (gp4_all, n_g), (sec_all, n_s)):
        assert bool(torch.isnan(whole[n:]).all())
    val, pads = decode(sec, 2 * C, Ho, Wo)
    assert bool(torch.isfinite(gp4).all()) and bool(torch.isfinite(val.double()).all()) and not pads.view(torch.int16).any()


@gpu
def test_generic_kernel_split_mode_1x1():
    """conv.hip with split operands (algo 5: the 1x1 two-source layers): the staged input of either source."""
    from yond_public_amd.engine import _PackedConv
    N, C, H, W = 2, 64, 9, 37
    g, x, w, b = tame(5, N, 2 * C, H, W, C, k=1)
    plan = status_plan()
    pc = _PackedConv(plan.dev, w, b, 1, 1, [C, C])

    def launch(xc):
        dst = torch.full((N, H, W, pc.coutp), float('nan'), device=DEV)
        plan._conv(pc, xc[..., :C].contiguous().to(DEV), xc[..., C:].contiguous().to(DEV), N, H, W, dst, algo='split')
        return word(plan), dst.cpu()

    assert launch(x)[0] == 0
    for pos in positions(N, H, W, 2 * C):
        xc = x.clone()
        xc[pos] = 65000.0
        st, got = launch(xc)
        assert st == 0, pos
        a64 = xc.permute(0, 3, 1, 2).double()
        z = F.conv2d(a64, w.double())
        y, Ty = M.through_epilogue(M.threshold_conv(a64, w, z, 1, 2), z, None, b.double()[None, :, None, None])
        assert M.ratio_report(f"guard: generic split 1x1, 65000 at {pos}", got.permute(0, 3, 1, 2), y, Ty).max() <= M.FACTOR
        for bad in BAD:
            xc[pos] = bad
            assert launch(xc)[0] & 1, (pos, bad)


@gpu
@pytest.mark.parametrize("parts", [2, 1])
def test_decoder_gemm_staged_and_plane_inputs(parts):
    """K1 (the decoder GEMM): a bad element in `cur` or in `skip`, staged from [N][H][W][C] tensors (split operands); from planes
    the consumer cannot see it -- the producer of the planes has raised the flag -- and must not answer with a finite value."""
    from test_hip_conv import to_hp, to_sp
    from yond_public_amd.engine import _PackedConv
    c, h, w, N = 64, 9, 20, 2
    g = torch.Generator().manual_seed(31)
    cur, skip = torch.randn(N, h, w, 2 * c, generator=g), torch.randn(N, 2 * h, 2 * w, c, generator=g)
    wf = torch.randn(3 * c, c, 2, 2, generator=g) / (3 * c) ** 0.5
    bf = torch.randn(c, generator=g)
    plan = status_plan()
    pc = _PackedConv(plan.dev, wf, bf, 1, 1, [2 * c, c], shuffle=True)
    planes = to_sp if parts == 2 else to_hp

    def launch(cu, sk, fmt):
        dst = torch.full((N, 2 * h, 2 * w, c), float('nan'), device=DEV)
        if fmt:
            plan._conv(pc, planes(cu), planes(sk), N, h, w, dst, algo='split' if parts == 2 else 'half', in_fmt=1)
        else:
            plan._conv(pc, cu.to(DEV), sk.to(DEV), N, h, w, dst, algo='split')
        return word(plan), dst.cpu()

    for which in (0, 1):
        t = (cur, skip)[which]
        for pos in positions(*t.shape):
            for bad in (65000.0,) + BAD:
                tc = t.clone()
                tc[pos] = bad
                args = (tc, skip) if which == 0 else (cur, tc)
                if parts == 2:
                    st, got = launch(*args, 0)
                    assert (st & 1) == (bad != 65000.0), (which, pos, bad)
                st, got = launch(*args, 1)
                if bad == 65000.0:
                    assert st == 0 and bool(torch.isfinite(got).all())
                else:
                    print(f"[guard] decoder GEMM from planes (parts {parts}), {bad} in source {which} at {pos}: consumer status {st}, "
                          f"non-finite outputs {int((~torch.isfinite(got)).sum())}")
                    assert (st & 1) or not bool(torch.isfinite(got).all())


def one_hot_layer(seed, N, C, H, W, Co, pix, big=100.0, co=None):
    """A tame layer whose output exceeds 65504 at exactly ONE element: input 1000 at one pixel / channel, centre-tap weight `big`."""
    g, x, w, b = tame(seed, N, C, H, W, Co)
    w = w * 0.01
    n, yy, xx = pix
    ci, co = C - 1, Co - 1 if co is None else co
    x[n, yy, xx, ci] = 1000.0
    w[co, ci] = 0.0
    w[co, ci, 1, 1] = big
    return x, w, b, co


@gpu
@pytest.mark.parametrize("parts", [2, 1])
@pytest.mark.parametrize("C,N,H,W,where", [(64, 2, 17, 40, 'first'), (64, 2, 17, 40, 'last'), (32, 1, 37, 70, 'mid'), (128, 1, 9, 33, 'last'),
                                           (64, 3, 13, 11, 'last')])
def test_producer_raises_for_a_stored_plane_value(parts, C, N, H, W, where):
    """The split-plane / h-only-plane store: tame input, exactly one OUTPUT beyond 65504 -- the producer must raise the flag.  The
    same launch with the big weight at 60 (output 6.0e4) stays silent.  Then the planes go to a consumer with a fresh status word:
    it reads finished halves and cannot raise anything; its answer must at least not be finite (recorded below)."""
    from test_hip_conv import hp_decode, sp_decode, to_p4
    from yond_public_amd.engine import _PackedConv
    pix = {'first': (0, 0, 0), 'last': (N - 1, H - 1, W - 1), 'mid': (N // 2, H // 2, W // 2)}[where]
    algo = 'split' if parts == 2 else 'half'
    decode = (lambda t: sp_decode(t, N, C, H, W)[0]) if parts == 2 else (lambda t: hp_decode(t, N, C, H, W)[0].double())
    plan = status_plan()
    ones = torch.ones(N, C, device=DEV)
    for big, over in ((60.0, False), (100.0, True)):
        x, w, b, co = one_hot_layer(C + H, N, C, H, W, C, pix, big)
        # conv1 of a residual block as the data flow launches it: planes of 4 in, SiLU staged, FiLM, SiLU, halves out
        kw = dict(escale=ones, eshift=b.to(DEV)[None].expand(N, C).contiguous(), ebatch=1, pre_act=1, post_act=1, algo=algo)
        pc = _PackedConv(plan.dev, w, None, 3, 1, [C])
        y32 = torch.full((N, H, W, C), float('nan'), device=DEV)
        plan._conv(pc, x.to(DEV), None, N, H, W, y32, **kw)
        assert word(plan) == 0                                      # (float32 output: nothing stored as halves)
        assert int((y32.abs() > 65504.0).sum()) == int(over) and float(y32[pix + (co,)].abs()) > 5.9e4
        out = plan._new_sp('t', N, H, W, C, parts)
        plan._conv(pc, to_p4(x), None, N, H, W, out, in_fmt=2, out_fmt=1, **kw)
        assert (word(plan) & 1) == int(over), (big, where)
        # the consumer: conv2 of the block, planes in (LDS-DMA), FiLM + residual in planes of 4, planes out
        g2, _, w2, b2 = tame(3, N, C, H, W, C)
        pc2 = _PackedConv(plan.dev, w2, None, 3, 1, [C])
        o2 = plan._new_sp('o', N, H, W, C, parts)
        plan._conv(pc2, out, None, N, H, W, o2, res=to_p4(x), in_fmt=1, out_fmt=1, res_fmt=2, escale=ones, eshift=kw['eshift'], ebatch=1, algo=algo)
        st2 = word(plan)
        fin = bool(torch.isfinite(decode(o2)).all())
        print(f"[guard] consumer of planes with one value {big * 1000:.0f} (parts {parts}, {where}): status {st2}, all finite {fin}")
        if over:
            assert (st2 & 1) or not fin
        else:
            assert st2 == 0 and fin


@gpu
@pytest.mark.parametrize("parts", [2, 1])
@pytest.mark.parametrize("C,N,H,W,where", [(32, 2, 37, 70, 'first'), (32, 2, 37, 70, 'last'), (64, 1, 23, 45, 'mid')])
def test_producer_raises_for_the_second_output(parts, C, N, H, W, where):
    """dst2 of the stride-2 layer: the first output is float32 planes of 4 (any magnitude), the second SiLU(value) as halves."""
    from test_hip_conv import to_hp, to_sp
    from yond_public_amd.engine import _PackedConv
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    opix = {'first': (0, 0, 0), 'last': (N - 1, Ho - 1, Wo - 1), 'mid': (N // 2, Ho // 2, Wo // 2)}[where]
    pix = (opix[0], 2 * opix[1], 2 * opix[2])                       # the centre tap of output (y, x) reads input (2 y, 2 x)
    algo = 'split' if parts == 2 else 'half'
    plan = status_plan()
    for big, over in ((60.0, False), (100.0, True)):
        x, w, b, co = one_hot_layer(C + W, N, C, H, W, 2 * C, pix, big)
        pc = _PackedConv(plan.dev, w, b, 3, 2, [C])
        xin = (to_sp if parts == 2 else to_hp)(x)
        gp4 = torch.full((N * 2 * C * Ho * Wo,), float('nan'), device=DEV)
        plan._conv(pc, xin, None, N, H, W, gp4, algo=algo, in_fmt=1, out_fmt=2)
        assert word(plan) == 0
        assert int((gp4.abs() > 65504.0).sum()) == int(over)
        second = plan._new_sp('second', N, Ho, Wo, 2 * C, parts)
        plan._conv(pc, xin, None, N, H, W, gp4, algo=algo, in_fmt=1, out_fmt=2, dst2=second)
        assert (word(plan) & 1) == int(over), (big, where)


# output pixels (n, y, x) of the 9 x 33 output of an 18 x 66 input, two images: the first; the last valid pixel of the ragged row and column
# tiles; the second row of row group 3 at lane 31 of a full tile; an interior pixel
TALL_PIXELS = [(0, 0, 0), (1, 8, 32), (0, 7, 31), (1, 4, 17)]


@gpu
@pytest.mark.parametrize("first_channel", [True, False], ids=["channel_0", "last_channel"])
@pytest.mark.parametrize("opix", TALL_PIXELS, ids=lambda p: "n%d_y%d_x%d" % p)
def test_s2_tall_guard_single_element(opix, first_channel):
    """The raising site of conv_s2_tall.hip (descriptor algo 7, two-image form, 128 -> 256): tame input, exactly ONE output element at 6.0e4 (silent)
    or at 1.0e5 (raised) -- with the second output only: planes of 4 are float32.  The template runs on the same input in a second status slot: the
    words and both outputs are equal."""
    from test_hip_conv import to_sp
    from test_hip_s2_tall import bits, run_pair
    from yond_public_amd.engine import _PackedConv
    C, Co, N, H, W = 128, 256, 2, 18, 66
    pix = (opix[0], 2 * opix[1], 2 * opix[2])                       # the centre tap of output (y, x) reads input (2 y, 2 x)
    plan = status_plan()
    for big, over in ((60.0, False), (100.0, True)):
        x, w, b, co = one_hot_layer(C + opix[2], N, C, H, W, Co, pix, big, co=0 if first_channel else None)
        pc = _PackedConv(plan.dev, w, b, 3, 2, [C])
        xin = to_sp(x)
        for d2 in (False, True):
            out = run_pair(plan, pc, xin, N, H, W, Co, d2, 0)       # (asserts the tags: the template in slot 0, /tall in slot 1)
            torch.cuda.synchronize()
            st = plan.status.cpu()
            plan.status.zero_()
            plan.status_slot = 0
            want = int(over and d2)
            assert (int(st[0]), int(st[1])) == (want, want), (opix, co, big, d2, st)
            gp4 = out[True][0]
            assert int((gp4.abs() > 65504.0).sum()) == int(over) and float(gp4.abs().max()) > 5.9e4
            assert torch.equal(bits(out[True][0]), bits(out[False][0]))
            if d2:
                assert torch.equal(bits(out[True][1]), bits(out[False][1]))


@gpu
@pytest.mark.parametrize("where", ['first', 'last'])
def test_s2_tall_guard_survives_the_tile_walk(where):
    """256 -> 512, output 40 x 224: 280 tiles on 256 persistent workgroups.  The single 1.0e5 element at the first / the last output pixel, both tile
    orders: in one order of each the element lies in a tile whose workgroup goes on to a second tile -- the maximum lives across tiles -- and all
    four launches raise the flag and equal the template."""
    from test_hip_conv import to_sp
    from test_hip_s2_tall import bits, run_pair
    from yond_public_amd.engine import _PackedConv
    C, Co, N, H, W = 256, 512, 1, 80, 448
    Ho, Wo = H // 2, W // 2
    opix = (0, 0, 0) if where == 'first' else (0, Ho - 1, Wo - 1)
    x, w, b, co = one_hot_layer(7, N, C, H, W, Co, (0, 2 * opix[1], 2 * opix[2]), 100.0)
    plan = status_plan()
    pc = _PackedConv(plan.dev, w, b, 3, 2, [C])
    xin = to_sp(x)
    for order in (0, 1):
        out = run_pair(plan, pc, xin, N, H, W, Co, True, order)
        torch.cuda.synchronize()
        st = plan.status.cpu()
        plan.status.zero_()
        assert (int(st[0]), int(st[1])) == (1, 1), (where, order, st)
        assert int((out[True][0].abs() > 65504.0).sum()) == 1
        assert torch.equal(bits(out[True][0]), bits(out[False][0])) and torch.equal(bits(out[True][1]), bits(out[False][1]))


@gpu
@pytest.mark.parametrize("kernel", ['stationary', 's2_tall'])
def test_stationary_and_tall_consumers_of_a_bad_plane_value(kernel):
    """The sibling of test_decoder_gemm_staged_and_plane_inputs for the two kernels written after the template (descriptor algo 6 and 7, no
    second output): consumers of finished planes.  One input element of 7.0e4, inf or NaN stored into the planes: the consumer raises nothing of
    its own (the producer of the planes has), and its output is not all finite; with 65000 it is finite and within the float64 bound."""
    from test_hip_conv import from_p4, nchw, nhwc, sp_decode, to_sp
    from test_hip_split_stress import check, dec_eval, dec_threshold
    from yond_public_amd.engine import _PackedConv
    N = 2
    g = torch.Generator().manual_seed(37)
    plan = status_plan()
    if kernel == 'stationary':
        c, h, w = 64, 9, 20
        srcs = [torch.randn(N, h, w, 2 * c, generator=g), torch.randn(N, 2 * h, 2 * w, c, generator=g)]
        wf = torch.randn(3 * c, c, 2, 2, generator=g) / (3 * c) ** 0.5
        bf = torch.randn(c, generator=g)
        pc = _PackedConv(plan.dev, wf, bf, 1, 1, [2 * c, c], shuffle=True)
        tag = "conv_split_kernel<k1,64,2>/stationary"
    else:
        C, H, W = 64, 18, 40
        srcs = [torch.randn(N, H, W, C, generator=g)]
        wf = torch.randn(2 * C, C, 3, 3, generator=g) / (3 * C ** 0.5)
        bf = torch.randn(2 * C, generator=g)
        pc = _PackedConv(plan.dev, wf, bf, 3, 2, [C])
        tag = "conv_split_kernel<2,64,2>/tall"

    def launch(ts):
        plan.prof = []
        if kernel == 'stationary':
            dst = torch.full((N * c * 4 * h * w,), float('nan'), device=DEV)
            plan._conv(pc, to_sp(ts[0]), to_sp(ts[1]), N, h, w, dst, algo='split', in_fmt=1, out_fmt=2, stationary=True)
            shape = (N, 2 * h, 2 * w, c)
        else:
            dst = torch.full((N * 2 * C * (H // 2) * (W // 2),), float('nan'), device=DEV)
            plan._conv(pc, to_sp(ts[0]), None, N, H, W, dst, algo='split', in_fmt=1, out_fmt=2, s2_tall=True)
            shape = (N, H // 2, W // 2, 2 * C)
        tags, plan.prof = [pr[0] for pr in plan.prof], None
        assert tags == [tag], tags
        return word(plan), from_p4(dst, *shape)

    def bound(ts):
        """(y, T) [N][H][W][C] from the values the planes hold."""
        dec = [nhwc(sp_decode(to_sp(t), *((N, t.shape[3]) + tuple(t.shape[1:3])))[0]) for t in ts]
        if kernel == 'stationary':
            z = dec_eval(dec[0], dec[1], wf.double())
            Tz = dec_threshold(dec[0], dec[1], wf.double(), z, 2)
            y = z + bf.double()
            return y, Tz + 2.0 ** -24 * (z.abs() + y.abs())
        a64 = nchw(dec[0])
        z = F.conv2d(a64, wf.double(), stride=2, padding=1)
        y, Ty = M.through_epilogue(M.threshold_conv(a64, wf, z, 2, 2), z, None, bf.double()[None, :, None, None])
        return nhwc(y), nhwc(Ty)

    st, got = launch(srcs)
    assert st == 0 and bool(torch.isfinite(got).all())
    for which, t in enumerate(srcs):
        for pos in positions(*t.shape):
            for bad in (65000.0,) + BAD:
                tc = t.clone()
                tc[pos] = bad
                ts = [tc if i == which else s for i, s in enumerate(srcs)]
                st, got = launch(ts)
                if bad == 65000.0:
                    assert st == 0 and bool(torch.isfinite(got).all()), (kernel, which, pos)
                    y, Ty = bound(ts)
                    check(f"guard: {kernel} consumer, 65000 in source {which} at {pos}", got, y, Ty, ch_axis=3)
                else:
                    nf = int((~torch.isfinite(got)).sum())
                    print(f"[guard] {kernel} consumer of planes, {bad} in source {which} at {pos}: consumer status {st}, non-finite outputs {nf}")
                    assert st in (0, 1), (kernel, which, pos, bad, st)
                    assert nf > 0, (kernel, which, pos, bad)


@gpu
def test_wgrad_split_gradient_limit():
    """wgrad_split.hip stages 2^11 dy as a half and tests amax < 31.9: one |dy| of 31.0 is clean, of 33.0 (and NaN) is reported --
    at the first, the last and an interior element."""
    from yond_public_amd import _lib as L
    lib = L.load()
    N, cin, cout, H, W = 2, 32, 64, 13, 21
    g = torch.Generator().manual_seed(2)
    xd = torch.randn(N, H, W, cin, generator=g).to(DEV)
    dy = torch.randn(N, H, W, cout, generator=g).clamp(-4, 4)
    need = int(lib.yond_conv_wgrad_split_ws_bytes(N, H, W, cin, cout))
    ws = torch.zeros(need // 4, device=DEV)
    buf = torch.zeros(9 * cout * cin + cout, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)

    def run(d):
        status.zero_()
        L.check(lib.yond_conv_wgrad_split_f32(L.ptr(xd), L.ptr(d.to(DEV)), N, H, W, cin, cout, L.ptr(buf), 1, L.ptr(ws), need, L.ptr(status),
                                              L.stream()), "wgrad_split")
        torch.cuda.synchronize()
        return int(status.item())

    assert run(dy) == 0
    for pos in positions(N, H, W, cout):
        for v, want in ((31.0, 0), (-31.0, 0), (33.0, 1), (float('nan'), 1), (float('-inf'), 1)):
            d = dy.clone()
            d[pos] = v
            assert run(d) == want, (pos, v)


@gpu
def test_gemm_split_words_each_alone_at_the_edges():
    """gemm_split.hip: word 0 for x, word 1 for |w| >= 32, each alone, at the first / last / an interior element of a ragged pixel count."""
    from test_hip_train import _gemm_split
    P, c = 333, 96
    g = torch.Generator().manual_seed(4)
    w = torch.randn(c, c, generator=g) / 10
    x = torch.randn(P, c, generator=g)
    y = torch.empty(P, c, device=DEV)

    def run(xx, ww):
        xx, ww = xx.to(DEV), ww.to(DEV)
        return _gemm_split([(xx.data_ptr(), ww.data_ptr(), 1, 0, c, c, 1 << 30, c)], P, c, c, c, 0, 1 << 30, None, y, c)

    assert run(x, w) == 0
    for pos in ((0, 0), (P - 1, c - 1), (P // 2, c // 2)):
        for v, want in ((65000.0, 0), (7.0e4, 1), (float('inf'), 1), (float('nan'), 1)):
            xb = x.clone()
            xb[pos] = v
            assert run(xb, w) == want, (pos, v)
    for pos in ((0, 0), (c - 1, c - 1), (c // 2, c // 3)):
        for v, want in ((31.0, 0), (33.0, 2), (float('nan'), 2)):
            wb = w.clone()
            wb[pos] = v
            assert run(x, wb) == want, (pos, v)


@gpu
def test_device_weight_packer_flags_a_weight_out_of_range():
    """yond_pack_conv_split_weight_dev_f32 (conv_split.hip): one weight of [cout][cin][taps] replaced -- 65000 packs silently into finite halves (the largest
    is fp16(65000) = 64992), 7.0e4 / inf / NaN set the bit."""
    from yond_public_amd import _lib as L
    lib = L.load()
    cout, cin, tn = 64, 32, 64
    g = torch.Generator().manual_seed(8)
    w = torch.randn(cout, cin, 9, generator=g) / 17.0
    status = torch.zeros(1, dtype=torch.int32, device=DEV)

    def run(ww):
        status.zero_()
        dst = torch.zeros(cout * cin * 9, device=DEV)
        L.check(lib.yond_pack_conv_split_weight_dev_f32(L.ptr(ww.to(DEV)), cout, cin, 3, tn, 2, L.ptr(dst), L.ptr(status), L.stream()), "pack dev")
        torch.cuda.synchronize()
        return int(status.item()), dst.cpu()

    assert run(w)[0] == 0
    for pos in ((0, 0, 0), (cout - 1, cin - 1, 8), (cout // 2, cin // 2, 4)):
        for v, want in ((65000.0, 0), (-7.0e4, 1), (float('inf'), 1), (float('nan'), 1)):
            wb = w.clone()
            wb[pos] = v
            st, packed = run(wb)
            assert st == want, (pos, v)
            if not want:
                halves = packed.view(torch.float16).float()
                assert bool(torch.isfinite(halves).all()) and float(halves.abs().max()) == 64992.0      # fp16(65000)


# ---- network level --------------------------------------------------------------------------------------------------------------

def regain(sd, key, f):
    sd[key] = sd[key] * f
    bkey = key[:-len('weight')] + 'bias'
    if f > 1 and bkey in sd:
        sd[bkey] = sd[bkey] * f


def tripped_state_dict(aname, sd, site, G=1e6):
    """One tensor of the network ~G, its consumers scaled back: every other activation stays O(1)."""
    sd = {k: v.clone() for k, v in sd.items()}
    guided = not aname.startswith('unet')
    if guided:
        if site in ('level0', 'level3', 'last'):
            blk = {'level0': 'conv1', 'level3': 'conv4', 'last': 'conv9'}[site]
            regain(sd, blk + '.conv1.weight', G)
            regain(sd, blk + '.conv2.weight', 1 / G)
        elif site == 'down':
            # the level-0 block's output (the stride-2 layer's input and the last decoder level's skip tensor) ~G:
            # conv_in x G, and every consumer of that tensor x 1/G
            regain(sd, 'conv_in.weight', G)
            regain(sd, 'conv1.conv1.weight', 1 / G)
            regain(sd, 'pool1.conv.weight', 1 / G)
            c = sd['conv9.short_cut.0.weight'].shape[0]
            sd['conv9.short_cut.0.weight'][:, c:] *= 1 / G
        elif site == 'upv':
            regain(sd, 'conv5.conv2.weight', G)                    # the bottleneck block's output, the first decoder GEMM's input
            regain(sd, 'upv6.weight', 1 / G)
    else:
        k = {'level0': 1, 'down': 2, 'level3': 4, 'last': 9}.get(site)
        if k is not None:
            regain(sd, f'conv{k}_1.weight', G)                      # (LeakyReLU is homogeneous: the pair cancels)
            regain(sd, f'conv{k}_2.weight', 1 / G)
        else:
            regain(sd, 'conv5_2.weight', G)
            regain(sd, 'upv6.weight', 1 / G)
    return sd


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def forward(net, guided, x, t):
    with torch.no_grad():
        return net(x, t) if guided else net(x)


@gpu
@pytest.mark.parametrize("site", ['level0', 'down', 'level3', 'upv', 'last'])
@pytest.mark.parametrize("precision", ['fp32', 'fp16'])
@pytest.mark.parametrize("aname", ['gru32', 'snr32', 'unet32'])
def test_network_guard_at_depth(aname, precision, site):
    """One activation tensor ~1e6 at five depths ('down': the tensor the first stride-2 layer reads -- UNetSeeInDark pools, its first
    layer after the pool stands in; 'upv': the tensor the first decoder GEMM reads).  The forward must warn, be finite and EQUAL the
    forward of the precision='fp32-mfma' plan on the same weights; afterwards the plan is unguarded-fast again: plan.strict is False
    and its next forward launches the split-operand kernels (a plan packs its weights once, so it cannot be handed good weights: a
    good network right after must not warn)."""
    import yond_oracle as O
    from hip_common import ARCHS
    from yond_public_amd import archs as A
    from yond_public_amd import pipeline as P
    arch = dict(ARCHS[aname])
    guided = 'guided' in arch
    sd_good = O.procedural_state_dict(arch, 9)
    sd = tripped_state_dict(aname, sd_good, site)

    def make(state, prec):
        net = getattr(A, arch['name'])(dict(arch))
        net.load_state_dict(state)
        net = net.to(DEV).eval()
        net.precision = prec
        return net

    x = (torch.rand((1, 4, 64, 96), generator=torch.Generator().manual_seed(3)) * 0.9).to(DEV)
    t = torch.tensor(0.04).to(DEV)
    want = cached(('want', aname, site), lambda: forward(make(sd, 'fp32-mfma'), guided, x, t))      # (shared by the two precisions)
    assert bool(torch.isfinite(want).all())
    net = make(sd, precision)
    with warnings.catch_warnings(record=True) as wl:
        warnings.simplefilter("always")
        y = forward(net, guided, x, t)
    assert any("fp16's range" in str(w.message) for w in wl), "no range-guard warning"
    assert bool(torch.isfinite(y).all())
    assert torch.equal(y, want), float((y - want).abs().max())
    plan = P._plan_of(net, torch.device(DEV))
    assert plan.strict is False
    plan.prof = []
    with warnings.catch_warnings(record=True) as wl:
        warnings.simplefilter("always")
        y2 = forward(net, guided, x, t)
    tags, plan.prof = [p[0] for p in plan.prof], None
    assert any(tg.startswith("conv_split_kernel<") for tg in tags), tags       # the fast path was tried again
    assert any("fp16's range" in str(w.message) for w in wl) and torch.equal(y2, want)
    good = cached(('good', aname, precision), lambda: make(sd_good, precision))
    with warnings.catch_warnings(record=True) as wl:
        warnings.simplefilter("always")
        yg = forward(good, guided, x, t)
    assert not any("fp16's range" in str(w.message) for w in wl) and bool(torch.isfinite(yg).all())


@gpu
@pytest.mark.parametrize("site", ['down_convs.1', 'up_convs.0'])
def test_estimator_guard_at_an_encoder_and_a_decoder_site(site):
    """EstimatorPlan: conv1 of one encoder / one decoder stage regained by 1e6, its conv2 by 1e-6 -- warning, finite, equal to the
    fp32-mfma plan; the plan is not left strict and a good network right after does not warn."""
    import estnet_common as E
    sd_good = E.weights(E.MEAN_ARGS, 13)
    sd = {k: v.clone() for k, v in sd_good.items()}
    regain(sd, site + '.conv1.weight', 1e6)
    regain(sd, site + '.conv2.weight', 1e-6)
    x = torch.from_numpy(E.map_frame(4, (1, 64, 64)))[:, None].to(DEV)
    net = E.build(E.MEAN_ARGS, sd, "cuda")
    with warnings.catch_warnings(record=True) as wl:
        warnings.simplefilter("always")
        y = net(x)
    assert any("fp16's range" in str(w.message) for w in wl)
    assert bool(torch.isfinite(y).all())
    assert torch.equal(y, E.build(dict(E.MEAN_ARGS, precision='fp32-mfma'), sd, "cuda")(x))
    assert net.plan(x.device).strict is False
    with warnings.catch_warnings(record=True) as wl:
        warnings.simplefilter("always")
        yg = E.build(E.MEAN_ARGS, sd_good, "cuda")(x)
    assert not any("fp16's range" in str(w.message) for w in wl) and bool(torch.isfinite(yg).all())
