"""Float64 models of FBI_Net's training step (yond_public_amd/train.py: TrainStep._forward_fbi over csrc/fbinet_train.hip).

`grads64` and `Adam64` are the whole step -- fbinet_common.torch_model64 with autograd, the reference's loss, and Adam -- in which each PReLU can take a
FORCED branch mask (the branches another run took), so that gradients stay comparable when an input within rounding of zero falls on
the other side.  The per-kernel models give each entry's exact result and a per-element BOUND derived from the kernel's arithmetic:

  * a product of two float32 is exact (the fp32-input MFMA and fmaf round the running sum, not the product; a float64 product of two
    float32 is exact);
  * fp32 accumulation of n terms, in any order: at most n roundings of partial sums that never exceed S = sum |terms|, so
    |error| <= n u S / (1 - n u), u = 2^-24;
  * a float64 finish: the fixed-order float64 sum of at most 2^20 terms adds 2^-33 S at the very most, and the result is rounded to
    float32 once: u |result|.
"""
import numpy as np
import torch
import torch.nn.functional as F

from fbinet_common import MASKS

U = 2.0 ** -24
TAPS = {0: [(0, 1), (0, 3), (1, 0), (1, 4), (2, 2), (3, 0), (3, 4), (4, 1), (4, 3)],            # (row, column) in the 5x5, pad 2
        1: [(0, 0), (0, 2), (1, 1), (2, 0), (2, 2)],                                            # in the 3x3 at dilation 3, pad 3
        2: [(0, 0)]}                                                                            # a 1x1
GEOM = {0: (5, 1), 1: (3, 3), 2: (1, 1)}                                                        # (K, dilation)


def acc_bound(n, S):
    """fp32 accumulation of n exact products whose absolute values sum to S, any order."""
    return n * U * S / (1.0 - n * U)


def tap_offsets(tset):
    K, dil = GEOM[tset]
    return [((r - K // 2) * dil, (c - K // 2) * dil) for r, c in TAPS[tset]]


def shift(x, dy, dx):
    """x [N][H][W][C] -> x(. + (dy, dx)) with zeros outside the frame."""
    N, H, W, C = x.shape
    out = torch.zeros_like(x)
    ys, ye, xs, xe = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if ys < ye and xs < xe:
        out[:, ys:ye, xs:xe] = x[:, ys + dy:ye + dy, xs + dx:xe + dx]
    return out


# -- per-kernel models -------------------------------------------------------------------------------------------------------------
def wgrad_model(x, dz, tset, n_terms):
    """yond_fbi_wgrad_f32: (dW [taps][co][ci], db [co], bound dW, bound db).  n_terms: the pixels a workgroup accumulates in fp32
    (yond_fbi_wgrad_rows(N, H) * W); the workgroups' partial sums are then added in float64."""
    x, dz = x.double(), dz.double()
    dw, bw = [], []
    for dy, dx in tap_offsets(tset):
        xs = shift(x, dy, dx)
        dw.append(torch.einsum('nhwo,nhwi->oi', dz, xs))
        bw.append(torch.einsum('nhwo,nhwi->oi', dz.abs(), xs.abs()))
    dw, bw = torch.stack(dw), torch.stack(bw)
    db, bb = dz.sum((0, 1, 2)), dz.abs().sum((0, 1, 2))
    fin = 2.0 ** -33
    return dw, db, acc_bound(n_terms, bw) + fin * bw + U * dw.abs(), acc_bound(n_terms, bb) + fin * bb + U * db.abs()


def tapconv_model(x, w_taps, bias, tset):
    """z = sum_t W_t x(. + d_t) + b with w_taps [taps][co][ci]: (z, bound) -- fp32 accumulation of taps * ci products, then the bias."""
    x, w_taps = x.double(), w_taps.double()
    z = torch.zeros(x.shape[:3] + (w_taps.shape[1],), dtype=torch.float64)
    s = torch.zeros_like(z)
    for (dy, dx), wt in zip(tap_offsets(tset), w_taps):
        xs = shift(x, dy, dx)
        z = z + torch.einsum('nhwi,oi->nhwo', xs, wt)
        s = s + torch.einsum('nhwi,oi->nhwo', xs.abs(), wt.abs())
    if bias is not None:
        z, s = z + bias.double(), s + bias.double().abs()
    return z, acc_bound(w_taps.shape[0] * w_taps.shape[2] + 1, s) + U * z.abs()


def dgrad_weights(w_taps):
    """The data gradient dx = sum_t W_t^T dz(. - d_t) as the same tap convolution: tap t of the flipped, transposed weights is the
    transpose of tap (taps - 1 - t) -- the sets are point-symmetric."""
    return w_taps.flip(0).transpose(1, 2).contiguous()


def prelu_model(a, b, div, slope):
    """yond_fbi_prelu_f32: (u, y, bound u, bound y): one rounding for the sum, one for the division, one for the slope product."""
    a = a.double()
    s = slope.double()
    u = ((a + b.double()) if b is not None else a) / div
    y = torch.where(u > 0, u, u * s)
    bu = torch.zeros_like(u) if (b is None and div == 1) else (2 * U if b is not None else U) * u.abs()
    return u, y, bu, bu * torch.where(u > 0, torch.ones_like(u), s.abs().expand_as(u)) + U * y.abs()


def prelu_bwd_model(u, dy, div, slope, one_slope):
    """yond_fbi_prelu_bwd_f32 on the float32 input u it is given: (du, dslope, bound du, bound dslope)."""
    u, dy, s = u.double(), dy.double(), slope.double()
    pos = u > 0
    du = torch.where(pos, dy, dy * s) / div
    t = torch.where(pos, torch.zeros_like(u), dy * u)
    ds, sa = t.sum((0, 1, 2)), t.abs().sum((0, 1, 2))
    if one_slope:
        ds, sa = ds.sum().reshape(1), sa.sum().reshape(1)
    return du, ds, 2 * U * du.abs(), 2.0 ** -33 * sa + U * ds.abs()


def mosaic_of(x4):
    """packed [N][h][w][4] -> mosaic [N][2h][2w]."""
    N, h, w, _ = x4.shape
    return x4.reshape(N, h, w, 2, 2).permute(0, 1, 3, 2, 4).reshape(N, 2 * h, 2 * w)


def packed_of(m):
    N, H, W = m.shape
    return m.reshape(N, H // 2, 2, W // 2, 2).permute(0, 1, 3, 2, 4).reshape(N, H // 2, W // 2, 4)


def first_bwd_model(x4, dz):
    """yond_fbi_first_bwd_f32: (dW [8][nf], db [nf], bound dW, bound db): float64 sums of exact products."""
    m, dz = mosaic_of(x4.double())[..., None], dz.double()
    offs = [(k // 3 - 1, k % 3 - 1) for k in (0, 1, 2, 3, 5, 6, 7, 8)]
    dw = torch.stack([(dz * shift(m, dy, dx)).sum((0, 1, 2)) for dy, dx in offs])
    sa = torch.stack([(dz * shift(m, dy, dx)).abs().sum((0, 1, 2)) for dy, dx in offs])
    db, sb = dz.sum((0, 1, 2)), dz.abs().sum((0, 1, 2))
    return dw, db, 2.0 ** -33 * sa + U * dw.abs(), 2.0 ** -33 * sb + U * db.abs()


def out_bwd_model(f, w, b, oc, sigmoid, sv, x4, dpred4):
    """yond_fbi_out_bwd_f32: (df, dW [oc][nf], db [oc], bound df, bound dW, bound db).  g0 = d loss / d y0 carries the float32
    roundings of dpred x (one) and, with the sigmoid, of sv s (1 - s) (six operations and expf's 2 ulp: 10 u) and the error of the
    recomputed y0 (fp32 accumulation of nf + 1 terms) through |d/dy (s (1 - s))| <= 0.1; the sums over pixels are float64."""
    f, w, b, dp = f.double(), w.double().reshape(oc, -1), b.double(), mosaic_of(dpred4.double())
    nf = f.shape[-1]
    x = mosaic_of(x4.double()) if oc == 2 else None
    g0 = dp * x if oc == 2 else dp
    e0 = U * g0.abs() if oc == 2 else torch.zeros_like(g0)
    if sigmoid:
        y0 = torch.einsum('nhwc,c->nhw', f, w[0]) + b[0]
        ey = acc_bound(nf + 1, torch.einsum('nhwc,c->nhw', f.abs(), w[0].abs()) + b[0].abs())
        s = torch.sigmoid(y0)
        d = sv * s * (1 - s)
        e0 = e0 * d + g0.abs() * (10 * U * d + sv * 0.1 * ey)
        g0 = g0 * d
    g = [g0] + ([dp] if oc == 2 else [])
    e = [e0] + ([torch.zeros_like(dp)] if oc == 2 else [])
    df = sum(gi[..., None] * w[i] for i, gi in enumerate(g))
    ab = sum((gi.abs() + ei)[..., None] * w[i].abs() for i, (gi, ei) in enumerate(zip(g, e)))
    bdf = sum(ei[..., None] * w[i].abs() for i, ei in enumerate(e)) + 3 * U * ab
    dw = torch.stack([torch.einsum('nhw,nhwc->c', gi, f) for gi in g])
    bdw = torch.stack([torch.einsum('nhw,nhwc->c', ei + 2.0 ** -33 * gi.abs(), f.abs()) for gi, ei in zip(g, e)]) + U * dw.abs()
    db = torch.stack([gi.sum() for gi in g])
    bdb = torch.stack([(ei + 2.0 ** -33 * gi.abs()).sum() for gi, ei in zip(g, e)]) + U * db.abs()
    return df, dw, db, bdf, bdw, bdb


# -- the whole step ----------------------------------------------------------------------------------------------------------------
def forward64(args, sd, x, masks=None, acts=None):
    """fbinet_common.torch_model64 on float64 tensors `sd` (autograd flows into them).  masks: {slope name: bool [N][C][H][W]} -- the
    branch each PReLU takes (True: the identity) instead of its own input's sign; acts: a dict that receives every PReLU's input."""
    m = {k: torch.tensor(v, dtype=torch.float64) for k, v in MASKS.items()}
    L = int(args['num_of_layers'])

    def prelu(name, v):
        key = name + '.weight'
        if acts is not None:
            acts[key] = v.detach()
        pos = (v > 0) if masks is None else masks[key]
        return torch.where(pos, v, v * sd[key].reshape(1, -1, 1, 1))

    def rm(pre, v):
        r = pre + 'residual_module.'
        h = prelu(r + 'activation1', F.conv2d(v, sd[r + 'conv1_1by1.weight'], sd[r + 'conv1_1by1.bias']))
        return prelu(r + 'activation2', (v + F.conv2d(h, sd[r + 'conv2_1by1.weight'], sd[r + 'conv2_1by1.bias'])) / 2.0)
    x = x.double()
    n = prelu('new1.activation_new1', F.conv2d(x, sd['new1.new1.conv1.weight'] * m['new1'], sd['new1.new1.conv1.bias'], padding=1))
    o = rm('new1.', n)
    total = o
    for i in range(L - 1):
        pre, conv, pad, dil = ('new2.', 'new2', 2, 1) if i == 0 else (f'new_{i - 1}.', 'new3', 3, 3)
        n = prelu(pre + 'activation_new1', F.conv2d(n, sd[f'{pre}{conv}.conv1.weight'] * m[conv], sd[f'{pre}{conv}.conv1.bias'], padding=pad, dilation=dil))
        o = rm(pre, prelu(pre + 'activation_new2', (n + o) / 2.0))
        total = total + o
    f = rm('', prelu('activation', total / L))
    y = F.conv2d(f, sd['output_layer.weight'], sd['output_layer.bias'])
    if args['output_type'] == 'sigmoid':
        y = torch.cat([float(args['sigmoid_value']) * torch.sigmoid(y[:, :1]), y[:, 1:]], dim=1)
    return y[:, :1] * x + y[:, 1:] if args['res'] else y


def loss64(pred, target, charbonnier):
    d = pred - target.double()
    return torch.sqrt(d * d + 1e-6).mean() if charbonnier else d.abs().mean()


def grads64(args, sd, x, target, charbonnier, masks=None):
    """One forward + backward: (loss, {name: gradient}, {slope name: PReLU input}, prediction).  sd: {name: tensor}, any dtype."""
    p = {k: torch.as_tensor(v).double().clone().requires_grad_(True) for k, v in sd.items()}
    acts = {}
    pred = forward64(args, p, x, masks, acts)
    loss = loss64(pred, target, charbonnier)
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in p.items()}, acts, pred.detach()


class Adam64:
    """torch.optim.Adam's update (defaults: betas 0.9, 0.999, eps 1e-8, no weight decay) in float64."""

    def __init__(self, sd, lr):
        self.p = {k: torch.as_tensor(v).double().clone() for k, v in sd.items()}
        self.m = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.lr, self.t = lr, 0

    def step(self, grads):
        self.t += 1
        c1, c2 = 1 - 0.9 ** self.t, 1 - 0.999 ** self.t
        for k, g in grads.items():
            self.m[k] = 0.9 * self.m[k] + 0.1 * g
            self.v[k] = 0.999 * self.v[k] + 0.001 * g * g
            self.p[k] = self.p[k] - self.lr / c1 * self.m[k] / ((self.v[k] / c2).sqrt() + 1e-8)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()
