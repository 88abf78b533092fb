"""Device-side execution plan of the reference's blind-spot denoiser FBI_Net (archs/comp.py:264-648, case 'FBI_Net') on the HIP
kernels of csrc/fbinet.hip: a stack of masked convolutions on the full-resolution one-channel Bayer mosaic, blind (no noise level t),
with an affine output a * x + b.

    yond_fbi_first_f32   x -> n                       3x3 without its centre, 1 -> nf, one PReLU slope
    yond_fbi_rm_f32      n -> o,  sum = o             the residual module: two chained 1x1 GEMMs, both PReLUs
    (L - 1) x [ yond_fbi_tapconv_f32  (n, o) -> (n', o')   9 taps of a 5x5 (layer new2) or centre + corners at dilation 3 (new_i)
                yond_fbi_rm_f32       o' -> o,  sum += o ]
    yond_fbi_rm_f32      PReLU(sum / L) -> f          the prologue form, no sum
    yond_fbi_out_f32     f -> a * x + b  (or y)       nf -> 2 | 1, optional sigmoid on a, stored as packed Bayer

The weights stay unmasked in the module; the plan packs the LIVE taps only, which is the reference's `weight * mask` at every
forward (archs/comp.py:272, 285, 298).  Every product is exact fp32 on the fp32-input MFMA: `uses_half_operands()` is False, there
is no range guard.  Activations are [N][H][W][nf] float32 at mosaic resolution; five of them live during a forward.
"""
import numpy as np
import torch

from . import _lib as L
from .engine import DenoiserPlan, _np_ptr

ARG_KEYS = ('channel', 'output_channel', 'nf', 'mul', 'num_of_layers', 'case', 'output_type', 'sigmoid_value', 'res')


def check_args(args):
    """Refuse, naming the setting, what the HIP plan does not run.  Returns the precision."""
    for key in ARG_KEYS:
        if key not in args:
            raise L.YondHipError(f"FBI_Net: the arch section needs '{key}' (archs/comp.py:572-580)")
    if args['case'] != 'FBI_Net':
        raise L.YondHipError(f"FBI_Net: case must be 'FBI_Net', got case={args['case']!r} (the ablation cases case1 .. case7 of "
                             "archs/comp.py:389-557 are not built)")
    if int(args['channel']) != 1:
        raise L.YondHipError(f"FBI_Net: channel must be 1 (the one-channel Bayer mosaic), got channel={args['channel']}")
    if (bool(args['res']), int(args['output_channel'])) not in ((True, 2), (False, 1)):
        raise L.YondHipError(f"FBI_Net: (res, output_channel) must be (True, 2) -- a * x + b -- or (False, 1), got res={args['res']}, "
                             f"output_channel={args['output_channel']}")
    if int(args['mul']) != 1:
        raise L.YondHipError(f"FBI_Net: mul must be 1 (the residual modules' nf -> nf * mul -> nf GEMMs are built square), got mul={args['mul']}")
    if int(args['nf']) not in (32, 64):
        raise L.YondHipError(f"FBI_Net: nf must be 32 or 64 (the kernels' channel tiles), got nf={args['nf']}")
    if int(args['num_of_layers']) < 3:
        raise L.YondHipError(f"FBI_Net: num_of_layers must be >= 3 (new1, new2 and at least one dilated layer), got num_of_layers={args['num_of_layers']}")
    if args['output_type'] not in ('linear', 'sigmoid'):
        raise L.YondHipError(f"FBI_Net: output_type must be 'linear' or 'sigmoid', got output_type={args['output_type']!r}")
    prec = args.get('precision', 'fp32-mfma')
    if prec != 'fp32-mfma':
        raise L.YondHipError(f"FBI_Net: precision must be 'fp32-mfma' (this arch's default), got precision={prec!r}: the split-operand "
                             "and half forms of the sparse-tap convolution are not built")
    return prec


class FBINetPlan(DenoiserPlan):
    """Packs an FBI_Net's parameters once and runs forwards on packed-Bayer NHWC4 device tensors.  The methods the pipeline calls
    (begin_guard, overflowed, uses_half_operands, status) are DenoiserPlan's."""

    def __init__(self, module, device):
        args = module.args
        check_args(args)
        self._init_launcher(device, 'fp32-mfma')
        self.kind = 'FBI_Net'
        self.guided = False
        self.norm = False
        self.res = bool(args['res'])
        self.nf = int(args['nf'])
        self.layers = int(args['num_of_layers'])
        self.oc = int(args['output_channel'])
        self.sigmoid = args['output_type'] == 'sigmoid'
        self.sigmoid_value = float(args['sigmoid_value'])
        nf = self.nf
        sd = {k: v.detach().to('cpu', torch.float32).contiguous() for k, v in module.state_dict().items()}

        def dev(t):
            return t.contiguous().to(self.dev)

        def packed(fn, what, w, n, *extra):
            out = np.empty(n, np.float32)
            L.check(fn(_np_ptr(w.numpy()), nf, *extra, _np_ptr(out)), what)
            return torch.from_numpy(out).to(self.dev)

        def rm(prefix):
            r = prefix + 'residual_module.'
            w1, w2 = sd[r + 'conv1_1by1.weight'], sd[r + 'conv2_1by1.weight']
            if tuple(w1.shape) != (nf, nf, 1, 1) or tuple(w2.shape) != (nf, nf, 1, 1):
                raise L.YondHipError(f"FBI_Net: {r}conv*_1by1 must be {nf} -> {nf}, got {tuple(w1.shape)}, {tuple(w2.shape)}")
            return (packed(self.lib.yond_pack_fbi_rm_weight_f32, "yond_pack_fbi_rm_weight_f32", w1, nf * nf), dev(sd[r + 'conv1_1by1.bias']),
                    dev(sd[r + 'activation1.weight']),
                    packed(self.lib.yond_pack_fbi_rm_weight_f32, "yond_pack_fbi_rm_weight_f32", w2, nf * nf), dev(sd[r + 'conv2_1by1.bias']),
                    dev(sd[r + 'activation2.weight']))

        w = sd['new1.new1.conv1.weight']
        if tuple(w.shape) != (nf, 1, 3, 3):
            raise L.YondHipError(f"FBI_Net: new1.new1.conv1.weight must be ({nf}, 1, 3, 3), got {tuple(w.shape)}")
        self.first = (packed(self.lib.yond_pack_fbi_first_weight_f32, "yond_pack_fbi_first_weight_f32", w, 8 * nf),
                      dev(sd['new1.new1.conv1.bias']), dev(sd['new1.activation_new1.weight'].reshape(1)))
        self.rms = [rm('new1.')]
        self.taps = []                                         # (tap set, packed weights, bias, s1, s2) of new2, new_0 .. new_{L-3}
        for i in range(self.layers - 1):
            pre, conv, tset, k = ('new2.', 'new2', 0, 5) if i == 0 else (f'new_{i - 1}.', 'new3', 1, 3)
            w = sd[f'{pre}{conv}.conv1.weight']
            if tuple(w.shape) != (nf, nf, k, k):
                raise L.YondHipError(f"FBI_Net: {pre}{conv}.conv1.weight must be ({nf}, {nf}, {k}, {k}), got {tuple(w.shape)}")
            ntap = int(self.lib.yond_fbi_taps(tset))
            self.taps.append((tset, packed(self.lib.yond_pack_fbi_tap_weight_f32, "yond_pack_fbi_tap_weight_f32", w, ntap * nf * nf, tset),
                              dev(sd[f'{pre}{conv}.conv1.bias']), dev(sd[pre + 'activation_new1.weight']), dev(sd[pre + 'activation_new2.weight'])))
            self.rms.append(rm(pre))
        self.rm_last = rm('')
        self.act_last = dev(sd['activation.weight'])
        self.out_w = dev(sd['output_layer.weight'].reshape(self.oc, nf))
        self.out_b = dev(sd['output_layer.bias'])
        self.live_taps = [int(self.lib.yond_fbi_taps(t[0])) for t in self.taps]

    def _timed(self, tag, flops, launch):
        prof = self.prof
        if prof is None:
            return launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        prof.append((tag, flops, e0, e1))

    def _rm(self, p, v, npix, o_out, total, mode, pre_slope=None):
        lib, nf = self.lib, self.nf
        self._timed("fbi_rm_kernel", 4.0 * nf * nf * npix, lambda: L.check(
            lib.yond_fbi_rm_f32(L.ptr(v), nf, L.ptr(p[0]), L.ptr(p[1]), L.ptr(p[2]), L.ptr(p[3]), L.ptr(p[4]), L.ptr(p[5]), L.ptr(pre_slope),
                                self.layers if pre_slope is not None else 0, npix, L.ptr(o_out), L.ptr(total), mode, L.stream()), "yond_fbi_rm_f32"))

    def forward_nhwc4(self, x4, t_dev=None, ub=None):
        """x4: [N][h][w][4] float32 device tensor (packed Bayer) -> [N][h][w][4].  t_dev and ub are accepted and unused: the network is
        blind and does not normalise (the pipeline passes both to every plan)."""
        L.require_cuda(x4, "x")
        N, h, w, c4 = x4.shape
        if c4 != 4:
            raise L.YondHipError(f"input must be [N][h][w][4], got {tuple(x4.shape)}")
        lib, nf = self.lib, self.nf
        H, W = 2 * h, 2 * w
        npix = N * H * W
        n, n2, o, o2, total = (self._new(N, H, W, nf) for _ in range(5))
        fw, fb, fs = self.first
        self._timed("fbi_first_kernel", 2.0 * 8 * nf * npix, lambda: L.check(
            lib.yond_fbi_first_f32(L.ptr(x4), N, h, w, nf, L.ptr(fw), L.ptr(fb), L.ptr(fs), L.ptr(n), L.stream()), "yond_fbi_first_f32"))
        self._rm(self.rms[0], n, npix, o, total, 1)
        for (tset, wpk, b, s1, s2), rmp, ntap in zip(self.taps, self.rms[1:], self.live_taps):
            self._timed(f"fbi_tapconv_kernel<{tset}>", 2.0 * ntap * nf * nf * npix, lambda: L.check(
                lib.yond_fbi_tapconv_f32(L.ptr(n), L.ptr(o), tset, nf, L.ptr(wpk), L.ptr(b), L.ptr(s1), L.ptr(s2), N, H, W, L.ptr(n2), L.ptr(o2),
                                         L.stream()), "yond_fbi_tapconv_f32"))
            n, n2 = n2, n
            self._rm(rmp, o2, npix, o, total, 2)
        self._rm(self.rm_last, total, npix, o, None, 0, pre_slope=self.act_last)
        y4 = torch.empty_like(x4)
        self._timed("fbi_out_kernel", 2.0 * self.oc * nf * npix, lambda: L.check(
            lib.yond_fbi_out_f32(L.ptr(o), nf, L.ptr(self.out_w), L.ptr(self.out_b), self.oc, int(self.sigmoid), self.sigmoid_value,
                                 L.ptr(x4) if self.res else None, N, h, w, L.ptr(y4), L.stream()), "yond_fbi_out_f32"))
        return y4

    def forward_mosaic(self, x):
        """Plug-in surface: the reference's [N][1][H][W] mosaic -> [N][oc == 2 ? 1 : 1][H][W]; the mosaic <-> packed reshuffle is torch's."""
        L.require_cuda(x, "x")
        N, c, H, W = x.shape
        if c != 1 or H % 2 or W % 2 or H < 2 or W < 2:
            raise L.YondHipError(f"FBI_Net takes [N][1][H][W] with even H, W >= 2, got {tuple(x.shape)}")
        x4 = x.reshape(N, H // 2, 2, W // 2, 2).permute(0, 1, 3, 2, 4).reshape(N, H // 2, W // 2, 4).contiguous()
        y4 = self.forward_nhwc4(x4)
        return y4.reshape(N, H // 2, W // 2, 2, 2).permute(0, 1, 3, 2, 4).reshape(N, 1, H, W).contiguous()

    def flops(self, N, h, w):
        """Algorithmic FLOPs of one forward on a packed [N][h][w][4] frame (live taps only)."""
        nf = self.nf
        per_pixel = 8 * nf + sum(self.live_taps) * nf * nf + (self.layers + 1) * 2 * nf * nf + self.oc * nf
        return 2.0 * N * (2 * h) * (2 * w) * per_pixel
