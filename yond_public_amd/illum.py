"""Illuminance correction on the device (csrc/illum.hip, include/yond_hip.h M2): the ELD protocol's brightness alignment, which the
reference ships as data_process/__init__.py:139-171 (IlluminanceCorrect) beside ELD_Full_Dataset.  A frame exposed at 1 / ratio and
multiplied back by the ratio turns a black-level error of a fraction of a DN into a global brightness error; one least-squares gain
per frame between the clamped prediction and the unsaturated targets removes it before PSNR / SSIM:

    p = clamp(predict, 0, 1);  gain = dot(p[source != 1], source[source != 1]) / dot(p[source != 1], p[source != 1]);  out = gain * p

Two launches and no host read in between: `illum_sums` leaves the float64 sums [5][3] (four CFA groups and the frame: num, den, count)
on the device, the apply forms the float32 gain from them there.  mode 'cfa' (an extension, no reference) applies each CFA group's own
gain.  There is no CPU fallback.
"""
import torch

from . import _lib as L
from .isp import _frame

LAYOUTS = {'bayer': 0, 'packed4': 1, 'flat': 2}      # YOND_ILLUM_BAYER / _PACKED4 / _FLAT
MODES = {'frame': 0, 'cfa': 1}                       # YOND_ILLUM_FRAME / _CFA
ILLUM_CORR = ('off', 'frame', 'cfa')                 # the drivers' --illum-corr / the runfiles' pipeline.illum_corr
_WS = {}


def illum_corr_of(pipe):
    """pipe['illum_corr'] (the drivers' --illum-corr / the runfile's pipeline.illum_corr): 'off' (default), 'frame' or 'cfa'."""
    v = (pipe or {}).get('illum_corr', 'off')
    if v is False or v is None:                      # (YAML reads a bare `off` as False)
        v = 'off'
    if v not in ILLUM_CORR:
        raise L.YondHipError(f"illum_corr {v!r}: one of {ILLUM_CORR}")
    return v


def _workspace(device):
    """The per-workgroup partials of one device and stream (launches on one stream are ordered: one buffer serves them all)."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    if key not in _WS:
        _WS[key] = torch.empty(L.load().yond_illum_ws_bytes() // 8, dtype=torch.float64, device=device)
    return _WS[key]


def _layout_args(t, layout):
    if layout not in LAYOUTS:
        raise L.YondHipError(f"layout {layout!r}: one of {tuple(LAYOUTS)}")
    if layout == 'bayer':
        if t.dim() != 2:
            raise L.YondHipError(f"layout 'bayer' takes one Bayer frame [H][W], got shape {tuple(t.shape)}")
        return int(t.shape[1]), LAYOUTS[layout]
    return 0, LAYOUTS[layout]


def _pair(pred, source):
    pred = _frame(pred, "pred")
    source = _frame(source, "source")
    if source.device != pred.device:
        source = source.to(pred.device)
    if pred.shape != source.shape:
        raise L.YondHipError(f"illuminance correction: shapes differ, {tuple(pred.shape)} and {tuple(source.shape)}")
    return pred, source


def illum_sums(pred, source, layout='bayer'):
    """The device float64 tensor [5][3]: {sum p * source, sum p * p, count} over the unsaturated targets of the four groups of
    `layout` ('bayer': a frame [H][W], group (y & 1) * 2 + (x & 1); 'packed4': [...][4], group = last index; 'flat': group 0) and,
    in row 4, of the frame."""
    pred, source = _pair(pred, source)
    width, lay = _layout_args(pred, layout)
    sums = torch.empty((5, 3), dtype=torch.float64, device=pred.device)
    with torch.cuda.device(pred.device):
        L.check(L.load().yond_illum_sums_f32(L.ptr(pred), L.ptr(source), pred.numel(), width, lay, L.ptr(sums),
                                             L.ptr(_workspace(pred.device)), L.stream()), "yond_illum_sums_f32")
    return sums


def illum_apply(pred, sums, mode='frame', clip=False, out=None, layout='bayer'):
    """out = gain * clamp(pred, 0, 1) with the gain(s) of `sums` (illum_sums' tensor), optionally clipped at 1; out may be pred."""
    if mode not in MODES:
        raise L.YondHipError(f"mode {mode!r}: one of {tuple(MODES)}")
    pred = _frame(pred, "pred")
    width, lay = _layout_args(pred, layout)
    if not isinstance(sums, torch.Tensor) or sums.dtype != torch.float64 or sums.device != pred.device or tuple(sums.shape) != (5, 3) \
            or not sums.is_contiguous():
        raise L.YondHipError("sums must be illum_sums' contiguous float64 [5][3] tensor on the device of pred")
    if out is None:
        out = torch.empty_like(pred)
    elif L.require_cuda(out, "out").shape != pred.shape or out.device != pred.device:
        raise L.YondHipError(f"out must have the shape and device of pred, got {tuple(out.shape)} on {out.device}")
    with torch.cuda.device(pred.device):
        L.check(L.load().yond_illum_apply_f32(L.ptr(pred), pred.numel(), width, lay, L.ptr(sums), MODES[mode], int(bool(clip)),
                                              L.ptr(out), L.stream()), "yond_illum_apply_f32")
    return out


def illuminance_correct(pred, source, mode='frame', clip=False, out=None, layout='bayer'):
    """(out, sums) of one frame, both on the device and without a host read: illum_sums, then illum_apply.  NumPy input is uploaded."""
    pred, source = _pair(pred, source)
    sums = illum_sums(pred, source, layout)
    return illum_apply(pred, sums, mode, clip, out, layout), sums


def gains(sums):
    """Host read of illum_sums' tensor -> (total gain, [four group gains], total den, total count); the gains as the device forms
    them, float32(num / den)."""
    import numpy as np
    s = sums.detach().cpu().numpy()
    with np.errstate(divide='ignore', invalid='ignore'):
        g = (s[:, 0] / s[:, 1]).astype(np.float32)
    return float(g[4]), [float(v) for v in g[:4]], float(s[4, 1]), float(s[4, 2])


class IlluminanceCorrect(torch.nn.Module):
    """The reference's module (data_process/__init__.py:140-171) on the device: forward(predict, source) for [N][C][H][W], one gain per
    item over all its channels, a batch-1 source shared by every item, the output not clipped."""

    def forward(self, predict, source):
        predict, source = _frame(predict, "predict"), _frame(source, "source")
        if predict.dim() != 4 or source.dim() != 4 or predict.shape[1:] != source.shape[1:] or source.shape[0] not in (1, predict.shape[0]):
            raise L.YondHipError(f"IlluminanceCorrect: predict {tuple(predict.shape)} and source {tuple(source.shape)} do not pair up")
        output = torch.empty_like(predict)
        for i in range(predict.shape[0]):
            illuminance_correct(predict[i], source[i if source.shape[0] != 1 else 0], out=output[i], layout='flat')
        return output
