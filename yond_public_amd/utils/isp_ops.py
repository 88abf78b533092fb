"""Function seam of utils/isp_ops.py:57-71 -- Bayer <-> packed RGGB, bit-exact index permutations run
as HIP copy kernels.  NumPy in -> NumPy out (as the reference), device tensor in -> device tensor out -- :152-160, repair_bad_pixels, and :171-197, FastISP."""
import numpy as np
import torch

from .. import pipeline as _P


def _wrap(fn, x):
    if isinstance(x, np.ndarray):
        return fn(x).cpu().numpy()
    return fn(x)


def bayer2rggb(bayer):
    """utils/isp_ops.py:57-59: (H, W) -> (H/2, W/2, 4), channel = 2*dy + dx."""
    return _wrap(_P.bayer2rggb, bayer)


def rggb2bayer(rggb):
    """utils/isp_ops.py:61-63."""
    return _wrap(_P.rggb2bayer, rggb)


def bayer2rggbs(bayers):
    """utils/isp_ops.py:65-67 (batched torch version): (..., H, W) -> (-1, H/2, W/2, 4)."""
    H, W = bayers.shape[-2:]
    flat = bayers.reshape(-1, H, W)
    return torch.stack([_P.bayer2rggb(b) for b in flat])


def rggb2bayers(rggbs):
    """utils/isp_ops.py:69-71."""
    H, W, _ = rggbs.shape[-3:]
    flat = rggbs.reshape(-1, H, W, 4)
    return torch.stack([_P.rggb2bayer(r) for r in flat])


def repair_bad_pixels(raw, bad_points, method='median'):
    """utils/isp_ops.py:152-160: every listed (row, col) of the Bayer frame replaced by the 3x3 median of its own CFA plane, run by the
    HIP kernel (bpc.repair_bad_pixels).  A new array / tensor is returned; the reference also writes into `raw`.  The kernel works on
    float32: a NumPy frame is converted to float32 and the result back to its dtype.  That is exact for uint16 and float32 frames -- the
    median is then a selection of the input's own values -- while a float64 frame gets the median of its values ROUNDED to float32."""
    from .. import bpc as _bpc
    if isinstance(raw, np.ndarray):
        dev = torch.from_numpy(np.ascontiguousarray(raw, np.float32)).cuda()
        return _bpc.repair_bad_pixels(dev, bad_points, method).cpu().numpy().astype(raw.dtype, copy=False)
    return _bpc.repair_bad_pixels(raw, bad_points, method)


def FastISP(img4c, wb=None, ccm=None, gamma=2.2):
    """utils/isp_ops.py:171-197: packed [h][w][4] (R, G1, G2, B; a tensor's [0] is taken, :173-174) -> [H][W][3] RGB float NumPy in
    [0, 1], rendered by the HIP kernel (isp.fast_isp: float32, the reference returns float64)."""
    from .. import isp as _isp
    if torch.is_tensor(img4c):
        img4c = img4c[0].detach()
    return _isp.fast_isp(img4c, wb, ccm, gamma).cpu().numpy()
