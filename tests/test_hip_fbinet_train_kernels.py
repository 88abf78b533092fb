"""GPU: every entry of csrc/fbinet_train.hip alone (and the data gradient as TrainStep runs it: the forward tap kernel on flipped,
transposed weights), per element, against its float64 model's bound (tests/fbinet_train_model.py: exact products, fp32 accumulation of
n terms, float64 finish); one-hot gradients bit for bit; two calls of every reducing entry bit-equal.  Shapes: smaller than tile and
halo, a tile seam in x at 32 with three tile rows, no tile size dividing it."""
import ctypes as C

import numpy as np
import pytest
import torch

import fbinet_train_model as M

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHAPES = [(1, 6, 10), (2, 24, 40), (3, 38, 50)]


def env():
    from yond_public_amd import _lib as L
    from yond_public_amd import train as TR
    return L, L.load(), TR, TR._plan(DEV)


def rnd(shape, seed, scale=1.0, wide=False):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=g) * scale
    if wide:                                                   # a 1e4 dynamic range
        t = t * 10.0 ** (torch.rand(shape, generator=g) * 4.0 - 2.0)
    return t.float()


def ws_for(lib, nf, N, H, W):
    n = int(lib.yond_fbi_train_ws_bytes(nf, N, H, W))
    assert n > 0
    return torch.empty((n + 7) // 8, dtype=torch.float64, device=DEV)


def wgrad(L, lib, x, dz, tset):
    N, H, W, nf = x.shape
    taps = len(M.TAPS[tset])
    ws = ws_for(lib, nf, N, H, W)
    out = torch.full((taps * nf * nf + nf,), float('nan'), device=DEV)
    L.check(lib.yond_fbi_wgrad_f32(L.ptr(x), L.ptr(dz), tset, nf, N, H, W, L.ptr(out), L.ptr(ws), ws.numel() * 8, L.stream()), "yond_fbi_wgrad_f32")
    torch.cuda.synchronize()
    return out[:taps * nf * nf].view(taps, nf, nf).cpu(), out[taps * nf * nf:].cpu()


def dense(w_taps, tset):
    K = M.GEOM[tset][0]
    w = torch.zeros((w_taps.shape[1], w_taps.shape[2], K, K))
    for (r, c), wt in zip(M.TAPS[tset], w_taps):
        w[:, :, r, c] = wt
    return w


def dgrad(L, lib, TR, plan, dz, w_taps, tset):
    """The data gradient as TrainStep's backward runs it."""
    N, H, W, nf = dz.shape
    w = dense(w_taps, tset)
    if tset == 2:
        out = TR._conv_fwd(plan, w, None, 1, 1, [nf], [dz], N, H, W, role='dgrad', xf=lambda t: t[:, :, 0, 0].t().contiguous()[:, :, None, None])
    else:
        wf = w.flip(2, 3).transpose(0, 1).contiguous()
        pk = np.empty(len(M.TAPS[tset]) * nf * nf, np.float32)
        L.check(lib.yond_pack_fbi_tap_weight_f32(C.c_void_p(wf.numpy().ctypes.data), nf, tset, C.c_void_p(pk.ctypes.data)), "pack")
        out = TR._fbi_tapconv(plan, dz, tset, torch.from_numpy(pk).to(DEV), torch.zeros(nf, device=DEV), torch.full_like(dz, float('nan')))
    torch.cuda.synchronize()
    return out.cpu()


def ratio(got, want, bound):
    return float(((got.double() - want).abs() / bound.clamp_min(1e-300)).max())


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("tset", [0, 1, 2])
@pytest.mark.parametrize("nf", [32, 64])
def test_weight_and_data_gradient_within_the_models_bounds(nf, tset, shape, wide=False):
    L, lib, TR, plan = env()
    N, H, W = shape
    x, dz = rnd((N, H, W, nf), 100 + nf + tset, wide=wide), rnd((N, H, W, nf), 200 + nf + tset, 1e-2, wide=wide)
    wt = rnd((len(M.TAPS[tset]), nf, nf), 300 + tset, 0.1, wide=wide)
    xd, dzd = x.to(DEV), dz.to(DEV)
    dw, db = wgrad(L, lib, xd, dzd, tset)
    n_terms = int(lib.yond_fbi_wgrad_rows(N, H)) * W
    mw, mb, bw, bb = M.wgrad_model(x, dz, tset, n_terms)
    rw, rb = ratio(dw, mw, bw), ratio(db, mb, bb)
    dx = dgrad(L, lib, TR, plan, dzd, wt, tset)
    mx, bx = M.tapconv_model(dz, M.dgrad_weights(wt), None, tset)
    rx = ratio(dx, mx, bx)
    print(f"[fbinet_train] nf {nf} set {tset} {shape}{' wide' if wide else ''}: error / bound dW {rw:.3f} db {rb:.3f} dx {rx:.3f}")
    assert rw <= 1.0 and rb <= 1.0 and rx <= 1.0
    dw2, db2 = wgrad(L, lib, xd, dzd, tset)
    assert torch.equal(dw.view(torch.int32), dw2.view(torch.int32)) and torch.equal(db.view(torch.int32), db2.view(torch.int32))


def test_gradients_on_a_1e4_dynamic_range():
    test_weight_and_data_gradient_within_the_models_bounds(64, 0, (2, 24, 40), wide=True)
    test_weight_and_data_gradient_within_the_models_bounds(32, 1, (2, 24, 40), wide=True)


@pytest.mark.parametrize("tset,nf", [(0, 32), (1, 64), (2, 32)])
def test_one_hot_gradients_are_single_products_bit_for_bit(tset, nf):
    """dz nonzero at ONE pixel and output channel: dW_t[co] is the float32 product with x at the tap's pixel (zero outside the frame),
    every other row is zero, and dx holds exactly W_t^T dz at the pixels p + d_t -- the mirrored taps of the forward kernel
    it runs on.  Pixels: corners, each side of the x = 32 and y = 8 seams, interior."""
    L, lib, TR, plan = env()
    N, H, W = 1, 24, 40
    x, wt = rnd((N, H, W, nf), 7), rnd((len(M.TAPS[tset]), nf, nf), 8, 0.1)
    for k, (py, px) in enumerate([(0, 0), (23, 39), (5, 31), (5, 32), (7, 10), (8, 10), (12, 20)]):
        co, v = (5 * k + 3) % nf, np.float32(0.37 + 0.11 * k)
        dz = torch.zeros((N, H, W, nf))
        dz[0, py, px, co] = float(v)
        dw, db = wgrad(L, lib, x.to(DEV), dz.to(DEV), tset)
        dx = dgrad(L, lib, TR, plan, dz.to(DEV), wt, tset)
        want_w, want_x = torch.zeros_like(dw), torch.zeros_like(dx)
        for t, (dy, dx_) in enumerate(M.tap_offsets(tset)):
            if 0 <= py + dy < H and 0 <= px + dx_ < W:
                want_w[t, co] = x[0, py + dy, px + dx_] * v
                want_x[0, py + dy, px + dx_] = wt[t, co] * v       # (z(p) reads x(p + d_t): that pixel receives W_t^T dz(p))
        assert torch.equal(dw, want_w), (py, px)
        assert torch.equal(dx, want_x), (py, px)
        assert float(db[co]) == float(v) and int((db != 0).sum()) == 1


@pytest.mark.parametrize("shape", [(1, 5, 7), (3, 38, 50)])
@pytest.mark.parametrize("one_slope", [False, True])
@pytest.mark.parametrize("nf", [32, 64])
def test_prelu_forward_and_backward(nf, one_slope, shape):
    """Slopes negative, zero and positive; inputs with exact zeros (the slope's branch, no slope gradient); pixel counts no workgroup
    chunk divides (35 and 5700)."""
    L, lib, TR, plan = env()
    N, H, W = shape
    npix = N * H * W
    a, b, dy = rnd((N, H, W, nf), 1), rnd((N, H, W, nf), 2), rnd((N, H, W, nf), 3)
    a.view(-1)[::7] = 0.0
    b.view(-1)[::7] = 0.0
    slope = torch.tensor([-0.25]) if one_slope else torch.linspace(-0.4, 0.5, nf)
    if not one_slope:
        slope[nf // 2] = 0.0
    ws = ws_for(lib, nf, N, H, W)
    for bb, div in ((None, 1.0), (b, 2.0), (None, 3.0)):
        ad, bd, sd, dyd = a.to(DEV), (None if bb is None else bb.to(DEV)), slope.to(DEV), dy.to(DEV)
        u, y = torch.full_like(ad, float('nan')), torch.full_like(ad, float('nan'))
        keep_u = bb is not None or div != 1.0
        L.check(lib.yond_fbi_prelu_f32(L.ptr(ad), L.ptr(bd), div, L.ptr(sd), slope.numel(), nf, npix, L.ptr(u) if keep_u else None, L.ptr(y), L.stream()),
                "yond_fbi_prelu_f32")
        mu, my, bu, by = M.prelu_model(a, bb, div, slope)
        u = u if keep_u else ad
        assert bool(((u.cpu().double() - mu).abs() <= bu).all()) and bool(((y.cpu().double() - my).abs() <= by).all())
        outs = []
        for _ in range(2):
            du, ds = torch.full_like(ad, float('nan')), torch.full((slope.numel(),), float('nan'), device=DEV)
            L.check(lib.yond_fbi_prelu_bwd_f32(L.ptr(u), L.ptr(dyd), div, L.ptr(sd), slope.numel(), nf, npix, L.ptr(du), L.ptr(ds), L.ptr(ws),
                                               ws.numel() * 8, L.stream()), "yond_fbi_prelu_bwd_f32")
            torch.cuda.synchronize()
            outs.append((du.cpu(), ds.cpu()))
        mdu, mds, bdu, bds = M.prelu_bwd_model(u.cpu(), dy, div, slope, one_slope)
        assert bool(((outs[0][0].double() - mdu).abs() <= bdu).all())
        r = ratio(outs[0][1], mds, bds)
        print(f"[fbinet_train] prelu_bwd nf {nf} {'one slope' if one_slope else 'per channel'} {shape} div {div}: dslope error / bound {r:.3f}")
        assert r <= 1.0
        assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)) and torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))


@pytest.mark.parametrize("shape", [(2, 3, 5), (3, 19, 25)])
@pytest.mark.parametrize("nf", [32, 64])
def test_first_layer_backward(nf, shape):
    L, lib, TR, plan = env()
    N, h, w = shape
    x4 = torch.rand((N, h, w, 4), generator=torch.Generator().manual_seed(5))
    dz = rnd((N, 2 * h, 2 * w, nf), 6, 1e-2)
    ws = ws_for(lib, nf, N, 2 * h, 2 * w)
    x4d, dzd = x4.to(DEV), dz.to(DEV)
    outs = []
    for _ in range(2):
        dwb = torch.full((9 * nf,), float('nan'), device=DEV)
        L.check(lib.yond_fbi_first_bwd_f32(L.ptr(x4d), L.ptr(dzd), N, h, w, nf, L.ptr(dwb), L.ptr(ws), ws.numel() * 8, L.stream()),
                "yond_fbi_first_bwd_f32")
        torch.cuda.synchronize()
        outs.append(dwb.cpu())
    mw, mb, bw, bb = M.first_bwd_model(x4, dz)
    rw, rb = ratio(outs[0][:8 * nf].view(8, nf), mw, bw), ratio(outs[0][8 * nf:], mb, bb)
    print(f"[fbinet_train] first_bwd nf {nf} {shape}: error / bound dW {rw:.3f} db {rb:.3f}")
    assert rw <= 1.0 and rb <= 1.0
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


@pytest.mark.parametrize("shape", [(2, 3, 5), (3, 19, 25)])
@pytest.mark.parametrize("oc,sigmoid", [(2, 0), (2, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("nf", [32, 64])
def test_output_layer_backward(nf, oc, sigmoid, shape):
    L, lib, TR, plan = env()
    N, h, w = shape
    sv = 0.1
    x4 = torch.rand((N, h, w, 4), generator=torch.Generator().manual_seed(5))
    f, dp4 = rnd((N, 2 * h, 2 * w, nf), 6), rnd((N, h, w, 4), 7, 1e-3)
    wo, bo = rnd((oc, nf), 8, 0.3), rnd((oc,), 9, 0.5)
    ws = ws_for(lib, nf, N, 2 * h, 2 * w)
    fd, wod, bod, x4d, dp4d = (t.to(DEV) for t in (f, wo, bo, x4, dp4))
    outs = []
    for _ in range(2):
        df, dwb = torch.full_like(fd, float('nan')), torch.full((2 * nf + 2,), float('nan'), device=DEV)
        L.check(lib.yond_fbi_out_bwd_f32(L.ptr(fd), nf, L.ptr(wod), L.ptr(bod), oc, sigmoid, sv, L.ptr(x4d) if oc == 2 else None,
                                         L.ptr(dp4d), N, h, w, L.ptr(df), L.ptr(dwb), L.ptr(ws), ws.numel() * 8, L.stream()), "yond_fbi_out_bwd_f32")
        torch.cuda.synchronize()
        outs.append((df.cpu(), dwb.cpu()))
    mdf, mdw, mdb, bdf, bdw, bdb = M.out_bwd_model(f, wo, bo, oc, bool(sigmoid), sv, x4, dp4)
    df, dwb = outs[0]
    rf = ratio(df, mdf, bdf)
    rw = ratio(dwb[:oc * nf].view(oc, nf), mdw, bdw)
    rb = ratio(dwb[2 * nf:2 * nf + oc], mdb, bdb)
    print(f"[fbinet_train] out_bwd nf {nf} oc {oc} sigmoid {sigmoid} {shape}: error / bound df {rf:.3f} dW {rw:.3f} db {rb:.3f}")
    assert rf <= 1.0 and rw <= 1.0 and rb <= 1.0
    if oc == 1:
        assert float(dwb[nf:2 * nf].abs().max()) == 0.0 and float(dwb[2 * nf + 1]) == 0.0
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)) and torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))
