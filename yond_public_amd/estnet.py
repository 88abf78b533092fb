"""Device-side execution plan of the noise-estimation network EstUnet (archs/Unet.py:474-611) on the HIP kernels of
libyond_hip.so.

The reference runs EstUnet through torch.nn on one full-resolution Bayer plane [N][1][H][W] (YOND_SIDD.py:333-335, 362-364).
Here a forward is a fixed sequence of launches over NHWC float32 activations:

    yond_est_conv_in_f32 (1 -> nf, ReLU) -> conv2 -> [maxpool -> conv1 -> conv2] x (depth - 1)
      -> [transposed 2x2 as a pixel-shuffle GEMM (+ skip in its epilogue for 'add'; two-source conv1 for 'concat')
          -> conv1 -> conv2] x (depth - 1) -> yond_est_head_f32 (1x1, optional square, spatial mean)

Every 3x3 layer is the denoisers' convolution (`DenoiserPlan._conv`: split-operand fp16-MFMA products at fp32 accuracy by
default, the fp32-input MFMA kernels for 'fp32-mfma' and for the range guard's re-run), ReLU is LeakyReLU with slope 0 in its
epilogue, and the tensor between the two 3x3 layers of a level travels in split planes where both layers take them.
"""
import contextlib

import numpy as np
import torch

from . import _lib as L
from .engine import DenoiserPlan, _PackedConv, _rup, sp_plane_units, UNET_SP, SPLIT_PLANES, WINO_DEFAULT


class _PackedUpAdd(_PackedConv):
    """The decoder's transposed 2x2 layer when the skip tensor is ADDED to its output ('add' merge): the residual sits in the
    epilogue of the generic GEMM kernel (conv.hip); the split kernel's decoder GEMM has no residual, so this layer never takes it."""

    def split(self, *a, **k):
        return None


def check_args(args):
    """Refuse, naming the setting, what the HIP plan does not run.  Returns the normalised settings."""
    up_mode = args['up_mode']
    merge_mode = args['merge_mode']
    if up_mode not in ('transpose', 'upsample'):
        raise ValueError(f"\"{up_mode}\" is not a valid mode for upsampling. Only \"transpose\" and \"upsample\" are allowed.")
    if merge_mode not in ('concat', 'add'):
        raise ValueError(f"\"{merge_mode}\" is not a valid mode for merging up and down paths. Only \"concat\" and \"add\" are allowed.")
    if up_mode == 'upsample':
        raise L.YondHipError("EstUnet: up_mode 'upsample' is not built on the HIP path (only 'transpose')")
    if args['in_nc'] * args['nframes'] != 1:
        raise L.YondHipError(f"EstUnet: in_nc * nframes must be 1 (one Bayer plane, what IterDenoise feeds), got "
                             f"in_nc={args['in_nc']}, nframes={args['nframes']}")
    if args['use_type'] not in ('std', 'var'):
        raise L.YondHipError(f"EstUnet: use_type must be 'std' or 'var', got {args['use_type']!r}")
    if not 1 <= int(args['out_nc']) <= 4:
        raise L.YondHipError(f"EstUnet: out_nc must be 1..4 for the HIP head, got {args['out_nc']}")
    if int(args['depth']) < 1:
        raise L.YondHipError(f"EstUnet: depth must be >= 1, got {args['depth']}")
    prec = args.get('precision', 'fp32')
    if prec == 'fp16':
        raise L.YondHipError("EstUnet: precision 'fp16' is not built for the estimator (its output is a noise level, not an image): "
                             "use 'fp32' or 'fp32-mfma'")
    if prec not in ('fp32', 'fp32-mfma'):
        raise ValueError(f"precision must be 'fp32' or 'fp32-mfma', got {prec!r}")
    return prec


def check_shape(depth, H, W):
    """H and W must divide by 2^(depth-1): the reference raises at the merge otherwise (archs/comp.py:118-121)."""
    m = 2 ** (depth - 1)
    if H % m or W % m:
        raise L.YondHipError(f"EstUnet: input {H} x {W} does not divide by 2^(depth-1) = {m} (depth={depth}): the decoder's merge "
                             "needs matching sizes")


class EstimatorPlan(DenoiserPlan):
    """Packs an EstUnet's parameters once and runs forwards on [N][H][W] device planes.  Reuses the denoiser plan's convolution
    launcher, split-plane tensors and range guard."""

    def __init__(self, module, device):
        args = module.args
        self._init_launcher(device, check_args(args))
        self.kind = 'EstUnet'
        self.depth = int(args['depth'])
        self.merge = args['merge_mode']
        self.sq = args['use_type'] == 'var'
        self.pge = bool(args['pge'])
        self.out_nc = int(args['out_nc'])
        sd = {k: v.detach().to('cpu', torch.float32) for k, v in module.state_dict().items()}
        dev = self.dev
        nf = sd['down_convs.0.conv1.weight'].shape[0]
        self.nf = nf
        cp = _rup(nf)
        w0 = torch.zeros(cp, 9)
        w0[:nf] = sd['down_convs.0.conv1.weight'].reshape(nf, 9)
        b0 = torch.zeros(cp)
        b0[:nf] = sd['down_convs.0.conv1.bias']
        self.w_in, self.b_in, self.c_in = w0.to(dev).contiguous(), b0.to(dev).contiguous(), cp
        self.down = []
        for i in range(self.depth):
            pre = f'down_convs.{i}.'
            cout = sd[pre + 'conv2.weight'].shape[0]
            c1 = None if i == 0 else _PackedConv(dev, sd[pre + 'conv1.weight'], sd[pre + 'conv1.bias'], 3, 1, [sd[pre + 'conv1.weight'].shape[1]])
            c2 = _PackedConv(dev, sd[pre + 'conv2.weight'], sd[pre + 'conv2.bias'], 3, 1, [cout])
            self.down.append((c1, c2))
        self.up = []
        for j in range(self.depth - 1):
            pre = f'up_convs.{j}.'
            wt = sd[pre + 'upconv.weight']                          # ConvTranspose2d [ins][outs][2][2]
            outs = wt.shape[1]
            upc = (_PackedUpAdd if self.merge == 'add' else _PackedConv)(dev, wt, sd[pre + 'upconv.bias'], 1, 1, [wt.shape[0]], shuffle=True)
            splits = [outs, outs] if self.merge == 'concat' else [outs]
            c1 = _PackedConv(dev, sd[pre + 'conv1.weight'], sd[pre + 'conv1.bias'], 3, 1, splits)
            c2 = _PackedConv(dev, sd[pre + 'conv2.weight'], sd[pre + 'conv2.bias'], 3, 1, [outs])
            self.up.append((upc, c1, c2))
        wf = sd['conv_final.weight'].reshape(self.out_nc, -1)
        cf = _rup(wf.shape[1])
        wp = torch.zeros(self.out_nc, cf)
        wp[:, :wf.shape[1]] = wf
        self.w_head, self.b_head = wp.to(dev).contiguous(), sd['conv_final.bias'].to(dev).contiguous()
        self._ws = {}

    # -- workspaces ---------------------------------------------------------------------------------------------------------
    def _buf(self, key, shape, dtype=torch.float32):
        """A tensor kept per (key, shape) across forwards."""
        k = (key, tuple(shape), dtype)
        t = self._ws.get(k)
        if t is None:
            t = self._ws[k] = torch.empty(shape, dtype=dtype, device=self.dev)
        return t

    def _pair(self, lvl, c1, c2, s0, s1, N, h, w, dst):
        """conv1 -> ReLU -> conv2 -> ReLU.  The tensor between them has one reader: at split precision conv1 stores it in split
        planes and conv2 stages it by LDS-DMA alone (the same bits as staging the float32 tensor)."""
        sp = (UNET_SP and SPLIT_PLANES and not self.strict and getattr(self, 'conv_algo', WINO_DEFAULT) == 'split'
              and self.precision == 'fp32' and c1.split(2) is not None and c2.split(2) is not None
              and N * sp_plane_units(h, w) * 64 < 2 ** 31)
        tmp = self._new_sp(('t', lvl), N, h, w, c1.coutp) if sp else self._buf(('t', lvl), (N, h, w, c1.coutp))
        self._conv(c1, s0, s1, N, h, w, tmp, post_act=2, slope=0.0, out_fmt=1 if sp else 0)
        return self._conv(c2, tmp, None, N, h, w, dst, post_act=2, slope=0.0, in_fmt=1 if sp else 0)

    @contextlib.contextmanager
    def _timed(self, tag, flops, nbytes):
        """With self.prof a list (tools/estnet_bench.py): an event pair around the launch(es) inside, recorded as (tag, flops, e0, e1)
        with the launch's HBM bytes in self.prof_bytes[tag] (the convolutions record themselves in DenoiserPlan._conv)."""
        if self.prof is None:
            yield
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        yield
        e1.record()
        self.prof.append((tag, flops, e0, e1))
        self.__dict__.setdefault('prof_bytes', {})
        self.prof_bytes[tag] = self.prof_bytes.get(tag, 0.0) + nbytes

    # -- forward --------------------------------------------------------------------------------------------------------------
    def forward(self, x):
        """x: [N][H][W] float32 device tensor.  Returns the device tensor [N][out_nc] (pge) or [N][out_nc][H][W]; no host sync."""
        L.require_cuda(x, "x")
        if x.dim() != 3:
            raise L.YondHipError(f"EstimatorPlan.forward expects [N][H][W], got {tuple(x.shape)}")
        N, H, W = x.shape
        check_shape(self.depth, H, W)
        self._tile_order = 0
        lib, st = self.lib, L.stream()
        a = self._buf(('x', 0), (N, H, W, self.c_in))
        with self._timed('est_conv_in', 2.0 * 9 * self.nf * N * H * W, 4.0 * N * H * W * (1 + self.c_in)):
            L.check(lib.yond_est_conv_in_f32(L.ptr(x), N, H, W, self.c_in, L.ptr(self.w_in), L.ptr(self.b_in), L.ptr(a), st),
                    "yond_est_conv_in_f32")
        h, w = H, W
        skips = []
        cur = None
        for i, (c1, c2) in enumerate(self.down):
            y = self._buf(('y', i), (N, h, w, c2.coutp))
            if i == 0:
                cur = self._conv(c2, a, None, N, h, w, y, post_act=2, slope=0.0)
            else:
                cur = self._pair(i, c1, c2, cur, None, N, h, w, y)
            if i < self.depth - 1:
                skips.append(cur)
                pooled = self._buf(('x', i + 1), (N, h // 2, w // 2, cur.shape[-1]))
                with self._timed('maxpool2', 0.0, 4.0 * N * h * w * cur.shape[-1] * 1.25):
                    L.check(lib.yond_maxpool2_f32(L.ptr(cur), N, h, w, cur.shape[-1], L.ptr(pooled), st), "yond_maxpool2_f32")
                h, w = h // 2, w // 2
                cur = pooled
        for j, (upc, c1, c2) in enumerate(self.up):
            lvl = self.depth - 2 - j
            skip = skips[lvl]
            # buffers: the encoder's input and output tensors of the level are dead once the GEMM / conv1 have read them, so `up`
            # takes the input's buffer (when the shapes agree) and the level's output the skip's
            up = self._buf(('x', lvl), (N, 2 * h, 2 * w, upc.cout_real_p))
            if self.merge == 'add':
                self._conv(upc, cur, None, N, h, w, up, res=skip)           # up + down in the GEMM's epilogue
                s1 = None
            else:
                self._conv(upc, cur, None, N, h, w, up)
                s1 = skip                                                    # torch.cat((up, down), 1): conv1's second source
            h, w = 2 * h, 2 * w
            out = self._buf(('y', lvl), (N, h, w, c2.coutp))
            cur = self._pair(lvl, c1, c2, up, s1, N, h, w, out)
        if self.pge:
            res = self._buf('mean', (N, self.out_nc))
            part = self._buf('partial', (int(lib.yond_est_head_ws_bytes(N, self.out_nc)) // 8,), torch.float64)
        else:
            res = torch.empty((N, self.out_nc, H, W), dtype=torch.float32, device=self.dev)
            part = None
        with self._timed('est_head', 2.0 * self.nf * self.out_nc * N * H * W, 4.0 * N * H * W * (cur.shape[-1] + (0 if self.pge else self.out_nc))):
            L.check(lib.yond_est_head_f32(L.ptr(cur), N, H, W, cur.shape[-1], L.ptr(self.w_head), L.ptr(self.b_head), self.out_nc,
                                          int(self.sq), int(self.pge), L.ptr(res), L.ptr(part), st), "yond_est_head_f32")
        return res.clone() if self.pge else res

    def forward_checked(self, x, slot=3):
        """forward + the range guard: one read of the status word (a host sync); a staged activation outside fp16's range
        recomputes the forward on the fp32-input MFMA kernels."""
        guarded = self.uses_half_operands()
        if guarded:
            self.begin_guard(slot)
        out = self.forward(x)
        if guarded and self.overflowed(slot):
            import warnings
            warnings.warn("an activation left fp16's range (|a| > 65504) in the estimator's split-operand convolutions: "
                          "this forward is recomputed on the fp32-input MFMA kernels")
            self.strict = True
            try:
                out = self.forward(x)
            finally:
                self.strict = False
        return out

    def flops(self, N, H, W):
        """Algorithmic FLOPs of one forward (real, unpadded channels; SURVEY section 8d's rule)."""
        macs, h, w = 9 * self.nf * H * W, H, W
        for i, (c1, c2) in enumerate(self.down):
            if c1 is not None:
                macs += c1.macs_per_pixel * h * w
            macs += c2.macs_per_pixel * h * w
            if i < self.depth - 1:
                h, w = h // 2, w // 2
        for upc, c1, c2 in self.up:
            macs += upc.macs_per_pixel * h * w
            h, w = 2 * h, 2 * w
            macs += (c1.macs_per_pixel + c2.macs_per_pixel) * h * w
        macs += self.nf * self.out_nc * H * W
        return 2.0 * macs * N
