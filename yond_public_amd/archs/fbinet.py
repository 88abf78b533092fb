"""The reference's blind-spot denoiser FBI_Net (archs/comp.py:264-648) behind the `archs` plug-in surface: constructed from the
runfile's `arch` dict (keys channel, output_channel, nf, mul, num_of_layers, case, output_type, sigmoid_value, res, plus this project's
`precision`), with the reference's state_dict keys, shapes and ORDER (`load_weights(..., by_name=False)` and a strict load_state_dict
take a reference checkpoint; the masks are plain attributes there and in no state_dict), called as `net(x)` on the one-channel Bayer
mosaic [N][1][H][W], any even H, W >= 2.

As for the U-Nets, the nn.Module only HOLDS parameters: `forward` runs on the HIP kernels through `fbinet.FBINetPlan`; a CPU tensor or
a missing libyond_hip.so raises.  The weights stay unmasked; the plan packs the live taps only.
"""
import torch
import torch.nn as nn

from .. import _lib as L
from ..fbinet import FBINetPlan, check_args
from .unet import _HipDenoiser, _Holder


def _prelu(n):
    return nn.PReLU(n, 0)


class _Conv1(_Holder):
    """New1 / New2 / New3 (archs/comp.py:264-301): key `conv1`."""

    def __init__(self, cin, cout, k, pad, dil=1):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, kernel_size=k, padding=pad, dilation=dil)


class _ResidualModule(_Holder):
    """archs/comp.py:303-322: keys activation1, activation2, conv1_1by1, conv2_1by1 (in this order)."""

    def __init__(self, c):
        super().__init__()
        self.activation1 = _prelu(c)
        self.activation2 = _prelu(c)
        self.conv1_1by1 = nn.Conv2d(c, c, kernel_size=1)
        self.conv2_1by1 = nn.Conv2d(c, c, kernel_size=1)


class _New1Layer(_Holder):
    """archs/comp.py:375-383: new1, residual_module, activation_new1 -- PReLU(in_ch): ONE slope for the nf channels."""

    def __init__(self, cin, c):
        super().__init__()
        self.new1 = _Conv1(cin, c, 3, 1)
        self.residual_module = _ResidualModule(c)
        self.activation_new1 = _prelu(cin)


class _NewLayer(_Holder):
    """New2_layer / New3_layer (archs/comp.py:404-415, 482-493): new2 | new3, activation_new1, residual_module, activation_new2."""

    def __init__(self, c, name, k, pad, dil):
        super().__init__()
        setattr(self, name, _Conv1(c, c, k, pad, dil))
        self.activation_new1 = _prelu(c)
        self.residual_module = _ResidualModule(c)
        self.activation_new2 = _prelu(c)


class FBI_Net(_HipDenoiser):
    """archs/comp.py:568-648, case 'FBI_Net': forward(x) on [N][1][H][W] returns a * x + b for `res`, the 1-channel output otherwise."""

    def __init__(self, args=None):
        super().__init__()
        precision = check_args(args)
        self.args = args
        self.res = args['res']
        self.case = args['case']
        self.precision = precision
        self.norm = False
        self.nframes = 1
        nf, layers = int(args['nf']), int(args['num_of_layers'])
        self.num_layers = layers
        self.output_type = args['output_type']
        self.sigmoid_value = args['sigmoid_value']
        self.new1 = _New1Layer(1, nf)
        self.new2 = _NewLayer(nf, 'new2', 5, 2, 1)
        for i in range(layers - 2):
            self.add_module(f'new_{i}', _NewLayer(nf, 'new3', 3, 3, 3))
        self.residual_module = _ResidualModule(nf)
        self.activation = _prelu(nf)
        self.output_layer = nn.Conv2d(nf, int(args['output_channel']), kernel_size=1)
        self._plan = None
        self._plan_key = None

    def _get_plan(self, device):
        """As _HipDenoiser._get_plan (the parameters' versions are in the key), with this arch's plan."""
        plist = getattr(self, '_plist', None)
        if plist is None:
            plist = self._plist = list(self.parameters())
        key = (str(device), self.precision, tuple([p._version for p in plist]))
        if self._plan is None or self._plan_key != key:
            self._plan = FBINetPlan(self, device)
            self._plan_key = key
        return self._plan

    def forward(self, x):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise L.YondHipError("FBI_Net runs on the MI355X HIP kernels only: move the input (and the module) to a ROCm device; "
                                 "there is no CPU path")
        with torch.no_grad():
            return self._get_plan(x.device).forward_mosaic(x.contiguous().float())
