"""The noise-estimation network of the reference's `est_*` runfile sections (archs/Unet.py:474-611, built from archs/comp.py:35-126
and archs/modules.py:91): EstUnet, constructed from the section dict, with the reference's state_dict keys and shapes (so
`load_weights` and shipped estimator checkpoints load unchanged).

As for the denoisers, the nn.Module only HOLDS parameters: `forward` runs on the HIP kernels through `estnet.EstimatorPlan`; a
CPU tensor or a missing libyond_hip.so raises.
"""
import torch
import torch.nn as nn

from .. import _lib as L
from ..estnet import EstimatorPlan, check_args, check_shape
from .unet import _Holder


def _conv33(cin, cout):
    return nn.Conv2d(cin, cout, kernel_size=3, stride=1, padding=1)


class _DownConv(_Holder):
    # keys: conv1, conv2   (archs/comp.py:52-78; ReLU after each, MaxPool2d(2) on every level but the deepest)
    def __init__(self, cin, cout):
        super().__init__()
        self.conv1 = _conv33(cin, cout)
        self.conv2 = _conv33(cout, cout)


class _UpConv(_Holder):
    # keys: upconv, conv1, conv2   (archs/comp.py:81-126, up_mode 'transpose')
    def __init__(self, cin, cout, merge_mode):
        super().__init__()
        self.upconv = nn.ConvTranspose2d(cin, cout, kernel_size=2, stride=2)
        self.conv1 = _conv33(2 * cout if merge_mode == 'concat' else cout, cout)
        self.conv2 = _conv33(cout, cout)


class EstUnet(nn.Module):
    """archs/Unet.py:474-611: U-Net regressing the noise parameters from one Bayer plane.  forward(x [N][1][H][W]) returns, as
    the reference: pge True -> the spatial mean of the 1x1 head, squeezed ([out_nc] for N = 1, [N][out_nc] otherwise);
    pge False -> the map [N][out_nc][H][W]; use_type 'var' squares the head's output first."""

    def default_args(self):
        self.args = {'out_nc': 4, 'in_nc': 4, 'depth': 3, 'nf': 64, 'nframes': 1, 'res': False, 'up_mode': 'transpose',
                     'merge_mode': 'add', 'use_type': 'std', 'pge': True}

    def __init__(self, args=None):
        super().__init__()
        self.default_args()
        if args is not None:
            for key in args:
                self.args[key] = args[key]
        self.precision = check_args(self.args)
        self.up_mode, self.merge_mode = self.args['up_mode'], self.args['merge_mode']
        self.out_nc = self.args['out_nc']
        self.in_nc = self.args['in_nc'] * self.args['nframes']
        self.depth = self.args['depth']
        self.start_filts = self.args['nf']
        self.noiseSTD = nn.Parameter(data=torch.log(torch.tensor(0.5)))       # in the state_dict, never used (:541-542)
        down, outs = [], None
        for i in range(self.depth):
            ins = self.in_nc if i == 0 else outs
            outs = self.start_filts * (2 ** i)
            down.append(_DownConv(ins, outs))
        up = []
        for i in range(self.depth - 1):
            ins = outs
            outs = ins // 2
            up.append(_UpConv(ins, outs, self.merge_mode))
        self.conv_final = nn.Conv2d(outs, self.out_nc, kernel_size=1)
        self.down_convs = nn.ModuleList(down)                                  # (registered after conv_final, as in the reference:
        self.up_convs = nn.ModuleList(up)                                      #  the state_dict keeps its key order)
        self._reset_params()
        self._plan = None
        self._plan_key = None

    def _reset_params(self):
        # :583-591: xavier_normal on every Conv2d weight, zero bias (ConvTranspose2d keeps torch's default init)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.xavier_normal_(m.weight)
                nn.init.constant_(m.bias, 0)

    def _apply(self, fn, *a, **k):
        self._plan = None
        self._plist = None
        return super()._apply(fn, *a, **k)

    def plan(self, device):
        """Packed weights + launch plan, rebuilt when a parameter was written to."""
        plist = getattr(self, '_plist', None)
        if plist is None:
            plist = self._plist = list(self.parameters())
        key = (str(device), self.precision, tuple([p._version for p in plist]))
        if self._plan is None or self._plan_key != key:
            self._plan = EstimatorPlan(self, device)
            self._plan_key = key
        return self._plan

    def forward(self, x):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise L.YondHipError("EstUnet runs on the MI355X HIP kernels only: move the input (and the module) to a ROCm device; "
                                 "there is no CPU path")
        if x.dim() != 4 or x.shape[1] != 1:
            raise L.YondHipError(f"EstUnet expects [N][1][H][W] (one Bayer plane), got {tuple(x.shape)}")
        check_shape(self.depth, x.shape[2], x.shape[3])
        x = x.contiguous().float()
        with torch.no_grad():
            y = self.plan(x.device).forward_checked(x[:, 0].contiguous())
        return y.squeeze() if self.args['pge'] else y

