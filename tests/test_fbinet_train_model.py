"""CPU: the float64 models of FBI_Net's training step (tests/fbinet_train_model.py) against torch's own float64 autograd of conv2d /
prelu, their bounds against a float32 torch run, and the whole-step model against two steps of the reference trainer
(tests/golden/fbinet_train.npz)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fbinet_common as D
import fbinet_train_common as T
import fbinet_train_model as M


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def dense(w_taps, tset):
    """[taps][co][ci] -> OIHW with zeros at the dead taps."""
    K = M.GEOM[tset][0]
    w = torch.zeros((w_taps.shape[1], w_taps.shape[2], K, K), dtype=w_taps.dtype)
    for (r, c), wt in zip(M.TAPS[tset], w_taps):
        w[:, :, r, c] = wt
    return w


def conv_autograd(x, w_taps, b, dz, tset, dtype):
    """torch's conv2d + autograd on NHWC tensors: (z, dx, dW [taps][co][ci], db)."""
    K, dil = M.GEOM[tset]
    xn = x.to(dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    w = dense(w_taps.to(dtype), tset).requires_grad_(True)
    bb = b.to(dtype).clone().requires_grad_(True)
    z = F.conv2d(xn, w, bb, padding=(K // 2) * dil, dilation=dil)
    z.backward(dz.to(dtype).permute(0, 3, 1, 2))
    dw = torch.stack([w.grad[:, :, r, c] for r, c in M.TAPS[tset]])
    return M.nhwc(z.detach()), M.nhwc(xn.grad), dw, bb.grad


@pytest.mark.parametrize("tset", [0, 1, 2])
def test_tap_models_equal_autograd_and_bound_a_float32_run(tset):
    N, H, W, nf = 2, 10, 14, 32
    x, dz = rnd((N, H, W, nf), 1 + tset), rnd((N, H, W, nf), 11 + tset, 1e-2)
    wt, b = rnd((len(M.TAPS[tset]), nf, nf), 21 + tset, 0.1), rnd((nf,), 31, 0.05)
    z64, dx64, dw64, db64 = conv_autograd(x, wt, b, dz, tset, torch.float64)
    z, bz = M.tapconv_model(x, wt, b, tset)
    dx, bdx = M.tapconv_model(dz, M.dgrad_weights(wt), None, tset)
    dw, db, bdw, bdb = M.wgrad_model(x, dz, tset, N * H * W)
    for got, want in ((z, z64), (dx, dx64), (dw, dw64), (db, db64)):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    # the float32 run rounds its inputs first: the models are evaluated on the rounded values
    x32, dz32, wt32, b32 = (t.float() for t in (x, dz, wt, b))
    z32, dx32, dw32, db32 = conv_autograd(x32, wt32, b32, dz32, tset, torch.float32)
    z, bz = M.tapconv_model(x32, wt32, b32, tset)
    dx, bdx = M.tapconv_model(dz32, M.dgrad_weights(wt32), None, tset)
    dw, db, bdw, bdb = M.wgrad_model(x32, dz32, tset, N * H * W)
    for name, got, want, bound in (("z", z32, z, bz), ("dx", dx32, dx, bdx), ("dW", dw32, dw, bdw), ("db", db32, db, bdb)):
        ratio = float(((got.double() - want).abs() / bound).max())
        print(f"[fbinet_train_model] set {tset} {name}: float32 torch error / bound {ratio:.3f}")
        assert ratio <= 1.0, name


@pytest.mark.parametrize("one_slope", [False, True])
@pytest.mark.parametrize("two,div", [(False, 1), (True, 2), (False, 3)])
def test_prelu_models_equal_autograd(one_slope, two, div):
    shape, nf = (2, 5, 7, 32), 32
    a, b, dy = rnd(shape, 3), (rnd(shape, 4) if two else None), rnd(shape, 5)
    a[0, 0, 0, :4] = 0.0                                       # exact zeros: the slope's branch, no slope gradient
    if two:
        b[0, 0, 0, :4] = 0.0
    slope = torch.tensor([-0.3]) if one_slope else torch.linspace(-0.4, 0.5, nf, dtype=torch.float64)
    slope = slope.double()
    an, bn, sn = a.clone().requires_grad_(True), (b.clone().requires_grad_(True) if two else None), slope.clone().requires_grad_(True)
    un = ((an + bn) if two else an) / div
    yn = F.prelu(un.permute(0, 3, 1, 2), sn).permute(0, 2, 3, 1)
    yn.backward(dy)
    u, y, _, _ = M.prelu_model(a, b, div, slope)
    du, ds, _, _ = M.prelu_bwd_model(u, dy, div, slope, one_slope)
    assert torch.equal(y, yn.detach())
    assert float((du - an.grad).abs().max()) <= 1e-15 and (not two or torch.equal(an.grad, bn.grad))
    assert float((ds - sn.grad).abs().max()) <= 1e-12
    # float32: the same chain in torch float32 stays inside the bounds
    a32, b32, dy32, s32 = a.float(), (b.float() if two else None), dy.float(), slope.float()
    u32 = ((a32 + b32) if two else a32) / div
    y32 = torch.where(u32 > 0, u32, u32 * s32)
    u, y, bu, by = M.prelu_model(a32, b32, div, s32)
    assert bool(((u32.double() - u).abs() <= bu).all()) and bool(((y32.double() - y).abs() <= by).all())
    du, ds, bdu, bds = M.prelu_bwd_model(u32, dy32, div, s32, one_slope)
    du32 = torch.where(u32 > 0, dy32, dy32 * s32) / div
    assert bool(((du32.double() - du).abs() <= bdu).all())


@pytest.mark.parametrize("oc,sigmoid", [(2, False), (2, True), (1, False), (1, True)])
def test_edge_layer_models_equal_autograd(oc, sigmoid):
    N, h, w, nf, sv = 2, 3, 5, 32, 0.1
    x4 = torch.rand((N, h, w, 4), generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    dz, f = rnd((N, 2 * h, 2 * w, nf), 8), rnd((N, 2 * h, 2 * w, nf), 9)
    # first layer
    wf = rnd((nf, 1, 3, 3), 10).requires_grad_(True)
    bf = rnd((nf,), 11).requires_grad_(True)
    mask = torch.tensor(D.MASKS['new1'], dtype=torch.float64)
    z = F.conv2d(M.mosaic_of(x4)[:, None], wf * mask, bf, padding=1)
    z.backward(dz.permute(0, 3, 1, 2))
    dw, db, _, _ = M.first_bwd_model(x4, dz)
    live = [0, 1, 2, 3, 5, 6, 7, 8]
    assert float((dw.t() - wf.grad.reshape(nf, 9)[:, live]).abs().max()) <= 1e-12 and float(wf.grad[:, 0, 1, 1].abs().max()) == 0.0
    assert float((db - bf.grad).abs().max()) <= 1e-12
    # output layer
    wo, bo = rnd((oc, nf, 1, 1), 12, 0.2).requires_grad_(True), rnd((oc,), 13).requires_grad_(True)
    fn = f.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    dp4 = rnd((N, h, w, 4), 14)
    y = F.conv2d(fn, wo, bo)
    if sigmoid:
        y = torch.cat([sv * torch.sigmoid(y[:, :1]), y[:, 1:]], dim=1)
    pred = y[:, :1] * M.mosaic_of(x4)[:, None] + y[:, 1:] if oc == 2 else y
    pred.backward(M.mosaic_of(dp4)[:, None])
    df, dwo, dbo, bdf, bdw, bdb = M.out_bwd_model(f, wo.detach(), bo.detach(), oc, sigmoid, sv, x4, dp4)
    assert float((df - M.nhwc(fn.grad)).abs().max()) <= 1e-12
    assert float((dwo - wo.grad.reshape(oc, nf)).abs().max()) <= 1e-12 and float((dbo - bo.grad).abs().max()) <= 1e-12
    assert bool((bdf > 0).all()) and bool((bdw > 0).all()) and bool((bdb > 0).all())


@pytest.mark.parametrize("name", ["a", "b"])
def test_step_model_is_the_pinned_forward_with_its_autograd(name):
    """forward64 equals fbinet_common.torch_model64 (pinned to the reference by tests/golden/fbinet.npz) in value and gradient; a forced
    mask equal to the model's own branches changes nothing."""
    args, shape = D.CASES[name]
    shape = (1, 1, 12, 16)
    sd = D.weights(args, 5)
    x, tgt = D.case_input(shape, 6), D.case_input(shape, 7)
    loss, grads, acts, pred = M.grads64(args, sd, x, tgt, False)
    p = {k: torch.as_tensor(v).double().clone().requires_grad_(True) for k, v in sd.items()}
    ref = D.torch_model64(args, p, x)
    assert torch.equal(ref.detach(), pred)
    M.loss64(ref, tgt, False).backward()
    for k in p:
        assert torch.equal(p[k].grad, grads[k]), k
    assert list(acts) == T.prelu_names(args)
    masks = {k: M.nhwc(v) > 0 for k, v in acts.items()}
    loss2, grads2, _, _ = M.grads64(args, sd, x, tgt, False, masks={k: v.permute(0, 3, 1, 2) for k, v in masks.items()})
    assert loss2 == loss
    for k in grads:                                            # (the backward's thread order may differ: last bits)
        assert float((grads[k] - grads2[k]).abs().max()) <= 1e-13 * max(1e-30, float(grads[k].abs().max())), k


@pytest.mark.parametrize("name", ["lin", "sig", "nores"])
def test_step_model_reproduces_the_reference_trainer(golden, name):
    """Two steps of the model (float64 autograd, Adam64) against the reference's float64 run: losses and live-tap gradients to 1e-9 of
    their size, updated weights to the reference's own float32 - float64 gap; every PReLU takes the stored branch."""
    g = golden("fbinet_train")
    args, charb = T.CASES[name]
    seed = int(g[f"{name}/seed"])
    names = [str(k) for k in g[f"{name}/params"]]
    sd = T.weights(name, seed)
    assert sorted(sd) == sorted(names)
    opt = M.Adam64({k: sd[k] for k in names}, T.LR)
    for s in (1, 2):
        lr_img, hr_img = T.batch(seed, s - 1)
        loss, grads, acts, _ = M.grads64(args, opt.p, lr_img, hr_img, charb)
        assert np.array_equal(T.mask_bits({k: M.nhwc(v).numpy() for k, v in acts.items()}, T.prelu_names(args)), g[f"{name}/mask{s}"])
        ref_loss = float(g[f"{name}/loss{s}"]) + float(g[f"{name}_d64/loss{s}"])
        assert abs(loss - ref_loss) <= 1e-12
        got, segs = T.flat({k: v.numpy() for k, v in grads.items()}, names)
        ref = T.f64(g, f"{name}/g{s}")
        stat = g[f"{name}/stat{s}"]
        for (k, a, b), (gap_g, gap_w, gmax) in zip(segs, stat):
            assert np.abs(got[a:b] - ref[a:b]).max() <= 1e-9 * gmax + 1e-7 * gap_g, (s, k)
        for k, v in grads.items():
            assert float((v.numpy() * (1 - T.live_mask(k, v.shape))).__abs__().max()) == 0.0, k      # dead taps: no gradient
        opt.step(grads)
        gotw, _ = T.flat({k: v.numpy() for k, v in opt.p.items()}, names)
        refw = g[f"{name}/w{s}"].astype(np.float64)
        for (k, a, b), (gap_g, gap_w, gmax) in zip(segs, stat):
            assert np.abs(gotw[a:b] - refw[a:b]).max() <= 1.001 * gap_w + 1e-7 * np.abs(refw[a:b]).max(), (s, k)
