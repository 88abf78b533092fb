"""The reference's comparison denoiser DnCNN (archs/comp.py:3-33) behind the `archs` plug-in surface: constructed from the runfile's
`arch` dict (keys in_nc, out_nc, nf, depth, use_bn, res, plus this project's `precision`), with the reference's state_dict keys and
shapes (`dncnn.{i}.weight` ..., BatchNorm buffers included: `load_weights(..., by_name=False)` and a strict load_state_dict take a
reference checkpoint), called as `net(x)` on NCHW float32 tensors.

As for the U-Nets, the nn.Module only HOLDS parameters: `forward` runs on the HIP kernels through `dncnn.DnCNNPlan`; a CPU tensor or
a missing libyond_hip.so raises.
"""
import torch.nn as nn

from .. import _lib as L
from ..dncnn import BN_EPS_REFERENCE, DnCNNPlan, check_args
from .unet import _HipDenoiser, _Holder


class _Stack(nn.Sequential):
    """`dncnn`: the reference's nn.Sequential, as a parameter container (its forward raises: compute runs in dncnn.DnCNNPlan)."""
    forward = _Holder.forward


class DnCNN(_HipDenoiser):
    """archs/comp.py:3-33: 3x3 convolution + ReLU, (depth - 2) x [3x3 convolution (no bias), BatchNorm, ReLU], 3x3 convolution
    (no bias); forward(x) returns x - out for `res`, out otherwise."""

    def __init__(self, args=None):
        super().__init__()
        precision = check_args(args)
        self.args = args
        self.res = args['res']
        self.precision = precision
        self.norm = False
        self.nframes = 1
        nf, depth = int(args['nf']), int(args['depth'])
        layers = [nn.Conv2d(4, nf, kernel_size=3, padding=1, bias=True), nn.Identity()]
        for _ in range(depth - 2):
            layers.append(nn.Conv2d(nf, nf, kernel_size=3, padding=1, bias=False))
            if args['use_bn']:
                layers.append(nn.BatchNorm2d(nf, eps=BN_EPS_REFERENCE, momentum=0.95))
            layers.append(nn.Identity())
        layers.append(nn.Conv2d(nf, 4, kernel_size=3, padding=1, bias=False))
        self.dncnn = _Stack(*layers)                           # (nn.Identity at the ReLUs' indices: the state_dict keeps the reference's numbering)
        self._plan = None
        self._plan_key = None

    def _get_plan(self, device):
        """As _HipDenoiser._get_plan, with the BatchNorm buffers in the key (load_state_dict writes them in place) and the refusal of
        batch statistics at every call (.train() does not touch a parameter)."""
        if self.training and self.args['use_bn']:
            raise L.YondHipError("DnCNN: the module is in .train() mode and has BatchNorm layers: this forward is inference (call .eval(): the "
                                 "running statistics are folded into the convolutions' epilogues); batch statistics run in train.TrainStep")
        plist = getattr(self, '_plist', None)
        if plist is None:
            plist = self._plist = list(self.parameters()) + list(self.buffers())
        key = (str(device), self.precision, tuple([p._version for p in plist]))
        if self._plan is None or self._plan_key != key:
            self._plan = DnCNNPlan(self, device)
            self._plan_key = key
        return self._plan

    def forward(self, x):
        return self._run(x, None)
