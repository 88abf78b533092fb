"""Device-side execution plan of the reference's comparison denoiser DnCNN (archs/comp.py:3-33) on the HIP kernels of
libyond_hip.so: a straight stack of full-resolution 3x3 convolutions, blind (no noise level t), residual `x - out`.

    yond_conv_in_f32 (4 -> nf, bias, ReLU) -> (depth - 2) x [3x3 nf -> nf, no bias, eval-mode BatchNorm, ReLU]
      -> yond_conv3x3_out4_f32 (3x3 nf -> 4, no bias;  x - out  for res, out itself otherwise)

Every middle layer is the denoisers' convolution (`DenoiserPlan._conv`: split-operand fp16-MFMA products at fp32 accuracy by default,
the fp32-input MFMA kernels for 'fp32-mfma' and for the range guard's re-run; 'fp16' rounds the operands to half, algo 4).  ReLU is
LeakyReLU with slope 0 in the epilogue, BatchNorm (running statistics) is folded on the host, in float64, into the epilogue's
(escale, eshift):  escale = gamma / sqrt(running_var + eps),  eshift = beta - running_mean * escale.  This plan is inference:
a module in .train() mode with BatchNorm layers is refused here (batch statistics and their backward run in train.TrainStep only,
csrc/bn_train.hip).

The tensors between the layers are plain [N][H][W][nf] float32 (every kernel form of the 3x3 layers takes and stores them, on all
three precisions and on the guard's re-run); the split-plane producer / consumer forms exist for PAIRS of layers (one producer,
one consumer that stages nothing else), not for a chain in which every layer is both, so they are not used here.  The last layer
has its own kernel (csrc/conv3x3_out4.hip): fp32-exact on every precision, no range guard of its own.
"""
import numpy as np
import torch

from . import _lib as L
from .engine import DenoiserPlan, _PackedConv, _np_ptr

BN_EPS_REFERENCE = 1e-4               # archs/comp.py:22


def check_args(args):
    """Refuse, naming the setting, what the HIP plan does not run.  Returns the precision."""
    for key in ('in_nc', 'out_nc', 'nf', 'depth', 'use_bn', 'res'):
        if key not in args:
            raise L.YondHipError(f"DnCNN: the arch section needs '{key}' (archs/comp.py:7-13)")
    if int(args['in_nc']) != 4 or int(args['out_nc']) != 4:
        raise L.YondHipError(f"DnCNN: the HIP plan takes packed Bayer input and output (in_nc == out_nc == 4), got in_nc={args['in_nc']}, "
                             f"out_nc={args['out_nc']} (the reference's raw2rgb branch, out_nc 3 + pixel_shuffle, is not built)")
    if int(args['depth']) < 3:
        raise L.YondHipError(f"DnCNN: depth must be >= 3 (first layer, at least one middle layer, last layer), got {args['depth']}")
    nf = int(args['nf'])
    if nf % 32 != 0 or not 32 <= nf <= 128:
        raise L.YondHipError(f"DnCNN: nf must be 32, 64, 96 or 128 (the convolution kernels' channel tiles; the last layer holds up to 128 "
                             f"input channels' weights in LDS), got {nf}")
    prec = args.get('precision', 'fp32')
    if prec not in ('fp32', 'fp32-mfma', 'fp16'):
        raise ValueError(f"precision must be 'fp32', 'fp32-mfma' or 'fp16', got {prec!r}")
    return prec


def fold_batchnorm(gamma, beta, mean, var, eps):
    """Eval-mode BatchNorm as the epilogue's (escale, eshift), formed in float64 and rounded to float32 once each."""
    g, b, m, v = (np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, np.float64) for t in (gamma, beta, mean, var))
    scale = g / np.sqrt(v + np.float64(eps))
    shift = b - m * scale
    return scale.astype(np.float32), shift.astype(np.float32)


class DnCNNPlan(DenoiserPlan):
    """Packs a DnCNN's parameters once and runs forwards on NHWC4 device tensors.  The methods the pipeline and the stream drivers
    call (forward_nhwc4, forward_nchw, begin_guard, overflowed, uses_half_operands, image_max, status) are DenoiserPlan's."""

    def __init__(self, module, device):
        args = module.args
        check_args(args)
        self._init_launcher(device, getattr(module, 'precision', 'fp32'))
        self.kind = 'DnCNN'
        self.guided = False
        self.norm = False
        self.res = bool(args['res'])
        self.nf = int(args['nf'])
        self.depth = int(args['depth'])
        layers = list(module.dncnn)
        if module.training and any(isinstance(m, torch.nn.BatchNorm2d) for m in layers):
            raise L.YondHipError("DnCNN: the module is in .train() mode and has BatchNorm layers: this forward is inference (call .eval(): the "
                                 "running statistics are folded into the convolutions' epilogues); batch statistics run in train.TrainStep")
        dev = self.dev
        first, last = layers[0], layers[-1]
        self.conv_in_w, self.conv_in_b = self._pack_conv_in(first.weight, first.bias)
        self.mid = []                                          # (packed conv, escale or None, eshift or None)
        i = 2
        while i < len(layers) - 1:
            conv = layers[i]
            pc = _PackedConv(dev, conv.weight, None, 3, 1, [self.nf])
            es = et = None
            i += 1
            if isinstance(layers[i], torch.nn.BatchNorm2d):
                bn = layers[i]
                s, t = fold_batchnorm(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
                es, et = torch.from_numpy(s).to(dev), torch.from_numpy(t).to(dev)
                i += 1
            i += 1                                             # the ReLU
            self.mid.append((pc, es, et))
        w = last.weight.detach().to('cpu', torch.float32).contiguous().numpy()
        if w.shape != (4, self.nf, 3, 3):
            raise L.YondHipError(f"DnCNN: the last layer must be 3x3, {self.nf} -> 4, got weights {tuple(w.shape)}")
        packed = np.empty(36 * self.nf, np.float32)
        L.check(self.lib.yond_pack_conv3x3_out4_weight_f32(_np_ptr(w), self.nf, _np_ptr(packed)), "yond_pack_conv3x3_out4_weight_f32")
        self.w_last = torch.from_numpy(packed).to(dev)

    def _last(self, feat, x4, N, H, W, dst):
        """dst = x4 - conv(feat) (res) or conv(feat)."""
        prof = self.prof
        if prof is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        L.check(self.lib.yond_conv3x3_out4_f32(L.ptr(feat), self.nf, L.ptr(self.w_last), None, L.ptr(x4) if self.res else None,
                                               -1.0 if self.res else 1.0, N, H, W, L.ptr(dst), L.stream()), "yond_conv3x3_out4_f32")
        if prof is not None:
            e1.record()
            prof.append(("conv3x3_out4_kernel", 2.0 * 36 * self.nf * N * H * W, e0, e1))
        return dst

    def forward_nhwc4(self, x4, t_dev=None, ub=None):
        """x4: [N][H][W][4] float32 device tensor -> [N][H][W][4].  t_dev and ub are accepted and unused: the network is blind and
        does not normalise (the pipeline passes both to every plan)."""
        L.require_cuda(x4, "x")
        self._tile_order = 0
        N, H, W, c4 = x4.shape
        if c4 != 4:
            raise L.YondHipError(f"input must be [N][H][W][4], got {tuple(x4.shape)}")
        prof = self.prof
        a = self._new(N, H, W, self.nf)
        if prof is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        L.check(self.lib.yond_conv_in_f32(L.ptr(x4), None, N, H, W, self.nf, L.ptr(self.conv_in_w), L.ptr(self.conv_in_b), 0.0, L.ptr(a),
                                          0, L.stream()), "yond_conv_in_f32")
        if prof is not None:
            e1.record()
            prof.append(("conv_in_kernel", 2.0 * 36 * self.nf * N * H * W, e0, e1))
        b = self._new(N, H, W, self.nf)
        for pc, es, et in self.mid:
            self._conv(pc, a, None, N, H, W, b, escale=es, eshift=et, post_act=2, slope=0.0)
            a, b = b, a
        return self._last(a, x4, N, H, W, self._new(N, H, W, 4))

    def flops(self, N, H, W):
        """Algorithmic FLOPs of one forward."""
        return 2.0 * N * H * W * (36 * self.nf * 2 + 9 * self.nf * self.nf * len(self.mid))
