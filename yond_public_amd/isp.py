"""Raw -> sRGB on the device (csrc/isp.hip, include/yond_hip.h R1) and the sRGB block metrics: the host side of
utils/sidd_utils.py:156-277 (process_sidd_image) and utils/isp_ops.py:171-197 (FastISP).

The host computes what is per image, in float64 as the reference does: the four gains, cam2rgb = inv(cst @ rgb2xyz) with rows
normalised to sum 1, the flip flags of the Bayer pattern, and -- once -- the 255 thresholds t_k = (k / 255) ** 2.2 that turn the gamma
into a table search (code = #{k : t_k <= x}: trunc(max(x, 1e-8) ** (1 / 2.2) * 255) away from the thresholds).
Everything per pixel is the kernel's.  There is no CPU fallback.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L

BAYER, PACKED4 = 0, 1            # YOND_ISP_BAYER / YOND_ISP_PACKED4
SIDD, FAST = 0, 1                # YOND_ISP_SIDD / YOND_ISP_FAST
ORDERS = {'rgb': 0, 'bgr': 1}    # YOND_ISP_RGB / YOND_ISP_BGR

RGB2XYZ = np.array([[0.4124564, 0.3575761, 0.1804375],            # utils/sidd_utils.py:161-167
                    [0.2126729, 0.7151522, 0.0721750],
                    [0.0193339, 0.1191920, 0.9503041]])
SONY_CCM = np.array([[1.9712269, -0.6789218, -0.29230508],        # utils/isp_ops.py:190-192
                     [-0.29104823, 1.748401, -0.45735288],
                     [0.02051281, -0.5380369, 1.5175241]])
_FLIPS = {((1, 2), (2, 3)): (False, False), ((2, 1), (3, 2)): (True, False),       # flip_bayer (utils/sidd_utils.py:182-196)
          ((2, 3), (1, 2)): (False, True), ((3, 2), (2, 1)): (True, True)}
RGGB = [[1, 2], [2, 3]]
_THR = {}


def threshold_table():
    """t_k = (k / 255) ** 2.2 for k = 1 .. 255 (float64, host)."""
    return (np.arange(1, 256, dtype=np.float64) / 255.0) ** 2.2


def _thresholds(device):
    key = (device.type, device.index)
    if key not in _THR:
        _THR[key] = torch.from_numpy(threshold_table()).to(device)
    return _THR[key]


def cam2rgb(cst):
    """inv(cst @ rgb2xyz), every row divided by its sum (utils/sidd_utils.py:168-170)."""
    m = np.linalg.inv(np.matmul(np.asarray(cst, np.float64).reshape(3, 3), RGB2XYZ))
    return m / np.sum(m, axis=-1, keepdims=True)


def flip_flags(bayer_2by2):
    """(left-right, up-down) flips that bring `bayer_2by2` (1 = R, 2 = G, 3 = B) to RGGB; an unknown pattern raises (the reference
    drops into pdb, utils/sidd_utils.py:192-195)."""
    try:
        key = tuple(tuple(int(v) for v in row) for row in np.asarray(bayer_2by2).reshape(2, 2).tolist())
    except (TypeError, ValueError):
        key = None
    if key not in _FLIPS:
        raise ValueError(f"Unknown Bayer pattern {bayer_2by2!r}")
    return _FLIPS[key]


def _frame(x, name):
    """NumPy array / host tensor / device tensor -> contiguous float32 device tensor (a host input is uploaded: the reference's
    functions take NumPy)."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    if isinstance(x, torch.Tensor) and not x.is_cuda:
        if not torch.cuda.is_available():
            raise L.YondHipError(f"{name}: rendering needs a ROCm device (the HIP path has no CPU fallback)")
        x = x.detach().cuda()
    if isinstance(x, torch.Tensor) and (x.dtype != torch.float32 or not x.is_contiguous()):
        x = x.detach().to(torch.float32).contiguous()
    return L.require_cuda(x, name)


def _render(frame, H, W, flips, layout, gains, ccm, mode, order=None, gamma=None):
    lib = L.load()
    g = (C.c_double * 4)(*[float(v) for v in gains])
    m = (C.c_double * 9)(*[float(v) for v in np.asarray(ccm, np.float64).reshape(9)])
    out_u8 = torch.empty((H, W, 3), dtype=torch.uint8, device=frame.device) if order is not None else None
    out_f32 = torch.empty((H, W, 3), dtype=torch.float32, device=frame.device) if gamma is not None else None
    with torch.cuda.device(frame.device):
        thr = _thresholds(frame.device) if out_u8 is not None else None
        L.check(lib.yond_render_srgb(L.ptr(frame), H, W, int(flips[0]), int(flips[1]), layout, g, m, mode, L.ptr(thr), L.ptr(out_u8),
                                     ORDERS[order] if order is not None else 0, L.ptr(out_f32), float(gamma) if gamma is not None else 0.0,
                                     L.stream()), "yond_render_srgb")
    return out_u8 if out_u8 is not None else out_f32


def render_sidd(frame, bayer_2by2, wb, cst, order='bgr', ccm=None):
    """process_sidd_image (utils/sidd_utils.py:156-180) -> device uint8 [H][W][3], channels in `order` ('bgr': what the reference
    returns; 'rgb': what a PNG writer takes).  frame: Bayer [H][W] (NumPy or device tensor); wb: AsShotNeutral [[r, g, b]]; cst:
    ColorMatrix2 (3 x 3); ccm: the camera -> sRGB matrix itself instead of cam2rgb(cst)."""
    if order not in ORDERS:
        raise ValueError(f"order must be 'rgb' or 'bgr', got {order!r}")
    flips = flip_flags(bayer_2by2)
    frame = _frame(frame, "frame")
    if frame.dim() != 2:
        raise L.YondHipError(f"render_sidd takes one Bayer frame [H][W], got shape {tuple(frame.shape)}")
    wb = np.asarray(wb, np.float64).reshape(-1)
    gains = (1 / wb[0], 1 / wb[1], 1 / wb[1], 1 / wb[2])                       # red, green, green, blue (:171, :250-253)
    H, W = frame.shape
    return _render(frame, H, W, flips, BAYER, gains, cam2rgb(cst) if ccm is None else ccm, SIDD, order=order)


def _fast_gain(v):
    """A gain as NumPy's promotion rules apply it to the float32 frame (utils/isp_ops.py:181, 184): a Python scalar is taken as
    float32, a NumPy scalar keeps its own precision."""
    if isinstance(v, torch.Tensor):
        v = v.item()
    return float(np.float32(v)) if type(v) in (int, float) else float(v)      # (np.float64 subclasses float: exact types)


def fast_isp(img4c, wb=None, ccm=None, gamma=2.2):
    """FastISP (utils/isp_ops.py:171-197) -> device float32 [H][W][3] RGB in [0, 1].  img4c: packed [h][w][4] in R, G1, G2, B order."""
    img4c = _frame(img4c, "img4c")
    if img4c.dim() != 3 or img4c.shape[-1] != 4:
        raise L.YondHipError(f"fast_isp takes a packed frame [h][w][4], got shape {tuple(img4c.shape)}")
    gains = (2.0, 1.0, 1.0, 2.0) if wb is None else (_fast_gain(wb[0]), 1.0, 1.0, _fast_gain(wb[2]))
    if isinstance(ccm, torch.Tensor):
        ccm = ccm.detach().cpu().numpy()
    h, w = img4c.shape[:2]
    return _render(img4c, 2 * h, 2 * w, (False, False), PACKED4, gains, SONY_CCM if ccm is None else ccm, FAST, gamma=gamma)


def block_metrics_rgb(dn_u8, hr_u8, bh=256, bw=256):
    """Per-block sRGB PSNR (compare_psnr(.., data_range=255) over the block's three channels) and SSIM (calculate_ssim: the mean of
    the channels' SSIM, YOND_SIDD.py:712-717) of two uint8 [H][W][3] device images -> two float64 arrays (row-major block order)."""
    lib = L.load()
    nt = lib.yond_block_metrics_tiles(bh, bw)
    if nt == -2:
        raise L.YondHipError(f"block_metrics_rgb: a {bh} x {bw} block has more than 65535 tiles of 32 x 32 (the launch's limit: about 8160 x 8160)")
    if nt < 0:
        raise L.YondHipError(f"block_metrics_rgb: blocks of {bh} x {bw} are smaller than the 11 x 11 SSIM window")
    for t, name in ((dn_u8, "dn_u8"), (hr_u8, "hr_u8")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or not t.is_contiguous() or t.dim() != 3 or t.shape[-1] != 3:
            raise L.YondHipError(f"{name} must be a contiguous uint8 [H][W][3] tensor on a ROCm device")
    if dn_u8.shape != hr_u8.shape:
        raise L.YondHipError(f"block_metrics_rgb: shapes differ, {tuple(dn_u8.shape)} and {tuple(hr_u8.shape)}")
    H, W = dn_u8.shape[:2]
    nblk = (H // bh) * (W // bw)
    out = torch.empty((nblk, nt, 3, 2), dtype=torch.float64, device=dn_u8.device)
    with torch.cuda.device(dn_u8.device):
        L.check(lib.yond_block_metrics_rgb8(L.ptr(dn_u8), L.ptr(hr_u8), H, W, bh, bw, L.ptr(out), L.stream()), "yond_block_metrics_rgb8")
    s = out.sum(dim=1).cpu().numpy()                                           # [block][channel][2]
    mse = s[:, :, 0].sum(axis=1) / (3 * bh * bw)
    with np.errstate(divide='ignore'):
        psnr = 10 * np.log10(255.0 ** 2 / mse)
    ssim = (s[:, :, 1] / ((bh - 10) * (bw - 10))).mean(axis=1)
    return psnr, ssim


def save_png(path, rgb_u8):
    """Write an RGB uint8 [H][W][3] array (NumPy or tensor) as a PNG through PIL."""
    from PIL import Image
    a = rgb_u8.cpu().numpy() if isinstance(rgb_u8, torch.Tensor) else np.asarray(rgb_u8)
    Image.fromarray(np.ascontiguousarray(a, np.uint8), 'RGB').save(path, format='PNG')
