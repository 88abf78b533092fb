"""GPU: the decoder GEMM with stationary weights (csrc/gemm_k1_stationary.hip, descriptor algo 6) against a float64 MODEL, not against the
template: an error the two kernels share -- the packed-weight layout, the index of the per-image vectors -- passes the bit-for-bit tests of
tests/test_hip_k1_stationary.py.  Reference: dec_eval (tests/test_hip_split_stress.py) in float64 on the values decoded from the input planes,
every output element against its own bound |got - ref| <= 4 T (dec_threshold, tests/split_model.py).  Operands as in the bit-for-bit test:
stress activations with values planted at fp16's subnormal boundary, heavy-tailed weights, a chunk of the skip tensor that holds 6e4 behind
zero weights; one output channel has zero weights and must hold the bias path bit for bit.  (C0, C1) = (64, 32) in the two-sub-positions form
with the [N][H][W][C] store, (128, 64) and (256, 128) with the planes-of-4 store; (h, w) = (1, 33) -- one pixel into the second segment -- and
(9, 31), two images; the bias alone, a per-image scale + shift, the bias with a LeakyReLU; both tile orders.
Then: every tensor of a launch in the MIDDLE of a NaN-filled allocation (the kernel keeps a ring of global loads that is refilled across
segment boundaries and past the last segment: a stray read is a NaN in an accumulator, a stray store changes a fence), and the LDS room of the
per-image vectors at its limit of 16 images and one past it, where the engine keeps the template.  Every launch asserts its tag."""
import numpy as np
import pytest
import torch

import split_model as M
from test_hip_conv import DEV, from_p4, nchw, nhwc, sp_decode, to_sp
from test_hip_k1_stationary import T_
from test_hip_s2_tall_model import bias_path, fenced, fences_intact, films, plant, status_plan
from test_hip_split_stress import check, dec_eval, dec_threshold, epilogue

pytestmark = pytest.mark.gpu

CHANNELS = [(64, 32), (128, 64), (256, 128)]          # (C0, C1): low-resolution input, skip tensor = channels of an output pixel
SHAPES = [(1, 33), (9, 31)]
K1_TAG = "conv_split_kernel<k1,64,2>"


def packed(plan, wf, bf, c):
    """(packed layer, out_fmt): 32-channel output pixels in the two-sub-positions form with the [N][H][W][C] store, else planes of 4."""
    from yond_public_amd.engine import _PackedConv, _PackedUpSub2
    if c == 32:
        pc = _PackedUpSub2(plan.dev, T_(wf), T_(bf), c)
        assert pc.ok
        return pc, 0
    return _PackedConv(plan.dev, T_(wf), T_(bf), 1, 1, [2 * c, c], shuffle=True), 2


def operands(rng, c, N, h, w, kind='signed'):
    """cur [N][h][w][2c] and skip [N][2h][2w][c] in split planes, their decoded float64 values, folded weights [3c][c][2][2]."""
    cur = nhwc(T_(M.stress_acts(rng, (N, 2 * c, h, w), kind)))
    skip = nhwc(T_(M.stress_acts(rng, (N, c, 2 * h, 2 * w), kind)))
    if kind == 'tame':
        wf = (rng.standard_normal((3 * c, c, 2, 2)) / (3 * c) ** 0.5).astype(np.float32)
        wf[:, c - 2] = 0.0
    else:
        wf = M.stress_weights(rng, c, 3 * c, 2, zero_out=c - 2, fan_in=3 * c).transpose(1, 0, 2, 3).copy()       # [2c cur + c skip][c][2][2]
        wf[2 * c + 16:2 * c + 32] = 0.0               # a chunk of the skip tensor with zero weights and large finite data
        cur[..., 0:8] = plant()
        skip[:, 0, 0, c - 24:c - 16] = plant()
        skip[..., 16:32] = 6.0e4
        if c == 32:
            skip[..., 8:16] = 6.0e4                   # (the two-sub-positions form's own zero-weight chunk reads channels 0 .. 15 again)
    cin, sin = to_sp(cur), to_sp(skip)
    c64 = nhwc(sp_decode(cin, N, 2 * c, h, w)[0])
    s64 = nhwc(sp_decode(sin, N, c, 2 * h, 2 * w)[0])
    return cin, sin, c64, s64, wf


def launch(plan, pc, cin, sin, N, h, w, dst, out_fmt, order, tag=K1_TAG + "/stationary", **kw):
    plan._tile_order = 1 - order
    plan.prof = []
    plan._conv(pc, cin, sin, N, h, w, dst, algo='split', in_fmt=1, out_fmt=out_fmt, stationary=True, **kw)
    tags, plan.prof = [pr[0] for pr in plan.prof], None
    assert tags == [tag], tags


def reference(c64, s64, wf):
    z = dec_eval(c64, s64, T_(wf).double())
    return z, dec_threshold(c64, s64, T_(wf).double(), z, 2)


def verify(name, got, out_fmt, z, Tz, es_et, post, slope, N, h, w, c):
    """dst of one launch against the model: (y, T_y, values), all [N][C][2h][2w]."""
    y, Ty = epilogue(nchw(Tz), nchw(z), es_et[0], es_et[1], post, slope, None)
    val = nchw(got.cpu().reshape(N, 2 * h, 2 * w, c) if out_fmt == 0 else from_p4(got, N, 2 * h, 2 * w, c))
    assert bool(torch.isfinite(val).all()), name
    check(name, val, y, Ty)
    want = bias_path(es_et, post, slope, N, c - 2)[:, None, None].expand(N, 2 * h, 2 * w)
    assert torch.equal(val[:, c - 2].view(torch.int32), want.contiguous().view(torch.int32)), (name, "the zero-weight channel")
    return y, Ty, val


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("cc", CHANNELS, ids=lambda c: f"{c[0]}_{c[1]}")
def test_stationary_gemm_against_float64(cc, hw):
    (c0, c), (h, w), N = cc, hw, 2
    assert c0 == 2 * c
    rng = np.random.default_rng([59, c, h, w])
    cin, sin, c64, s64, wf = operands(rng, c, N, h, w)
    bf = (10.0 ** rng.uniform(-2, 2, c) * rng.choice([-1.0, 1.0], c)).astype(np.float32)
    z, Tz = reference(c64, s64, wf)
    plan = status_plan()
    pc, out_fmt = packed(plan, wf, bf, c)
    for fname, kw, es_et, post, slope in films(rng, N, c, bf):
        for order in (0, 1):
            got = torch.full((N * c * 4 * h * w,), float('nan'), device=DEV)
            launch(plan, pc, cin, sin, N, h, w, got, out_fmt, order, **kw)
            torch.cuda.synchronize()
            name = f"algo 6 c{c} N{N} {h}x{w} film={fname} order={order}"
            assert int(plan.status[0]) == 0, name
            verify(name, got, out_fmt, z, Tz, es_et, post, slope, N, h, w, c)


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("cc", CHANNELS, ids=lambda c: f"{c[0]}_{c[1]}")
def test_stationary_gemm_inside_nan_fences(cc, hw):
    """Tame data; both input plane tensors and dst each the middle of a NaN-filled allocation.  Lanes outside the image read the plane's zero
    unit and store beyond the buffer resource's extent; the look-ahead past the last segment reads the last segment's units again."""
    (c0, c), (h, w), N = cc, hw, 2
    rng = np.random.default_rng([61, c, h, w])
    cin, sin, c64, s64, wf = operands(rng, c, N, h, w, kind='tame')
    bf = rng.standard_normal(c).astype(np.float32)
    z, Tz = reference(c64, s64, wf)
    plan = status_plan()
    pc, out_fmt = packed(plan, wf, bf, c)
    cv, c_all = fenced(cin)
    sv, s_all = fenced(sin)
    for order in (0, 1):
        dv, d_all = fenced(torch.zeros(N * c * 4 * h * w))
        launch(plan, pc, cv, sv, N, h, w, dv, out_fmt, order)
        torch.cuda.synchronize()
        name = f"algo 6 in NaN fences c{c} {h}x{w} order={order}"
        assert int(plan.status[0]) == 0, name
        assert fences_intact(d_all) and fences_intact(c_all) and fences_intact(s_all), name
        assert torch.equal(cv.view(torch.int32), cin.view(torch.int32)) and torch.equal(sv.view(torch.int32), sin.view(torch.int32)), name
        verify(name, dv, out_fmt, z, Tz, (None, bf), 0, 0.0, N, h, w, c)


@pytest.mark.parametrize("N,stationary", [(16, True), (17, False)], ids=["at_the_limit", "one_past_it"])
def test_stationary_gemm_vector_room(N, stationary):
    """(128, 64) at 1 x 33 with a scale + shift pair per image: 16 images fill the kernel's LDS room for the vectors exactly -- the last image's
    last channel reads its last float -- and 17 do not fit: the engine keeps the template."""
    c, h, w = 64, 1, 33
    rng = np.random.default_rng([67, N])
    cin, sin, c64, s64, wf = operands(rng, c, N, h, w)
    z, Tz = reference(c64, s64, wf)
    es, et = M.stress_film(rng, N, c)
    plan = status_plan()
    pc, out_fmt = packed(plan, wf, np.zeros(c, np.float32), c)
    kw = dict(escale=T_(es).to(DEV), eshift=T_(et).to(DEV), ebatch=1)
    for order in (0, 1):
        dv, d_all = fenced(torch.zeros(N * c * 4 * h * w))
        launch(plan, pc, cin, sin, N, h, w, dv, out_fmt, order, tag=K1_TAG + ("/stationary" if stationary else ""), **kw)
        torch.cuda.synchronize()
        name = f"algo 6 vector room N{N} ({'/stationary' if stationary else 'template'}) order={order}"
        assert int(plan.status[0]) == 0 and fences_intact(d_all), name
        y, Ty, val = verify(name, dv, out_fmt, z, Tz, (es, et), 0, 0.0, N, h, w, c)
        check(name + ", last image, last channel", val[N - 1:, c - 1:], y[N - 1:, c - 1:], Ty[N - 1:, c - 1:])
        assert torch.equal(val[N - 1, c - 2], T_(et)[N - 1, c - 2].expand(2 * h, 2 * w)), name
