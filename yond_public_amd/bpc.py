"""Defective pixels on the device (csrc/bpc.hip, include/yond_hip.h M4): hot and dead pixels are not Poisson-Gaussian noise -- the VST
does not stabilise them, the denoiser keeps them as signal, and the low-light protocols multiply them by the digital gain.

`repair_bad_pixels` is the reference's utils/isp_ops.py:152-160 for device tensors: every listed (row, col) is replaced by the 3x3 median
of its own CFA plane (cv2.medianBlur's replicated border), the medians taken from the input frame.  `detect_and_repair` is THIS PROJECT'S
EXTENSION for frames without a calibrated list: a pixel that stands out from all eight same-colour neighbours by t standard deviations
of the noise model variance = beta1 * x + beta2 (what pipeline.SimpleNLF returns) is flagged and repaired in the same pass.  Two touching
same-colour defects hide each other: clusters need a list.  The rule's false-positive behaviour on real texture has been checked on
synthetic frames only.  There is no CPU fallback.
"""
import numpy as np
import torch

from . import _lib as L

TILE_H, TILE_W = 32, 128            # YOND_BPC_TILE_H / YOND_BPC_TILE_W: the detect kernel's tile (the tests place defects on its seams)
MAX_SAVED_POINTS = 4096             # coordinates the drivers keep per frame (--save sidecar)


def _mosaic(t, name):
    t = L.require_cuda(t, name)
    if t.dim() != 2 or t.shape[0] < 2 or t.shape[1] < 2 or t.shape[0] % 2 or t.shape[1] % 2 or t.numel() >= 2 ** 31:
        raise L.YondHipError(f"{name}: one Bayer frame [H][W] with even H and W and fewer than 2^31 pixels, got shape {tuple(t.shape)}")
    return t


def check_points(points, shape=None):
    """A host list of (row, col) as a contiguous int32 [n][2] array; with `shape`, every point must lie inside that frame."""
    pts = np.asarray(points)
    if pts.size == 0:
        return np.zeros((0, 2), np.int32)
    if pts.ndim != 2 or pts.shape[1] != 2 or not np.issubdtype(pts.dtype, np.integer):
        raise ValueError(f"bad points: an integer array [n][2] of (row, col), got shape {pts.shape} of {pts.dtype}")
    if shape is not None:
        bad = (pts[:, 0] < 0) | (pts[:, 0] >= shape[0]) | (pts[:, 1] < 0) | (pts[:, 1] >= shape[1])
        if bad.any():
            r, c = pts[bad][0]
            raise ValueError(f"bad points: ({r}, {c}) and {int(bad.sum()) - 1} more lie outside the {shape[0]} x {shape[1]} frame")
    elif np.abs(pts).max() >= 2 ** 31:
        raise ValueError("bad points: coordinates beyond int32")
    return np.ascontiguousarray(pts, np.int32)


def repair_bad_pixels(raw, bad_points, method='median'):
    """utils/isp_ops.py:152-160 for a device frame [H][W]: a new tensor, `raw` with the same-colour 3x3 median (of `raw`) at every point
    of bad_points.  bad_points: a host array / list of (row, col), each checked against the frame, or a device integer tensor [n][2],
    which is not read on the host -- the kernel skips a point outside the frame.  (The reference also writes into its argument.)"""
    if method != 'median':
        raise ValueError(f"method {method!r}: the reference implements 'median' alone")
    raw = _mosaic(raw, "raw")
    H, W = int(raw.shape[0]), int(raw.shape[1])
    if isinstance(bad_points, torch.Tensor) and bad_points.is_cuda:
        if bad_points.numel() and (bad_points.dim() != 2 or bad_points.shape[1] != 2 or bad_points.dtype not in (torch.int32, torch.int64)):
            raise L.YondHipError(f"bad_points: an int32 / int64 tensor [n][2], got {tuple(bad_points.shape)} of {bad_points.dtype}")
        pts = bad_points.reshape(-1, 2).to(device=raw.device, dtype=torch.int32).contiguous()
    else:
        if isinstance(bad_points, torch.Tensor):
            bad_points = bad_points.numpy()
        pts = torch.from_numpy(check_points(bad_points, (H, W))).to(raw.device)
    out = raw.clone()                                        # the one device copy; the launch writes n elements
    n = int(pts.shape[0])
    if n:
        with torch.cuda.device(raw.device):
            L.check(L.load().yond_bpc_repair_list_f32(L.ptr(raw), L.ptr(out), H, W, L.ptr(pts), n, L.stream()), "yond_bpc_repair_list_f32")
    return out


def detect_and_repair(frame, beta1, beta2, t=6.0, coords=0):
    """(out, info) of one device frame [H][W]: pixels that stand out from all eight same-colour neighbours by more than t standard
    deviations of variance = beta1 * x + beta2 (the frame's own units) are replaced by the 3x3 same-colour median of `frame`.
    info = {'hot': n, 'cold': n, 'points': None | sorted int32 [k][2], 'overflow': bool}: the counts are exact; with coords = cap > 0 up to
    cap coordinates (row, col) come back, sorted lexicographically, and overflow says that more were flagged than were kept.
    One launch and one host read (the counts)."""
    frame = _mosaic(frame, "frame")
    beta1, beta2, t, cap = float(beta1), float(beta2), float(t), int(coords or 0)
    if cap < 0:
        raise ValueError(f"coords {coords!r}: a capacity >= 0")
    H, W = int(frame.shape[0]), int(frame.shape[1])
    out = torch.empty_like(frame)
    counts = torch.zeros(2, dtype=torch.int32, device=frame.device)
    buf = torch.empty((cap, 2), dtype=torch.int32, device=frame.device) if cap else None
    with torch.cuda.device(frame.device):
        L.check(L.load().yond_bpc_detect_repair_f32(L.ptr(frame), L.ptr(out), H, W, beta1, beta2, t, L.ptr(counts), L.ptr(buf), cap, L.stream()),
                "yond_bpc_detect_repair_f32")
    hot, cold = (int(v) for v in counts.cpu().numpy().view(np.uint32))
    info = {'hot': hot, 'cold': cold, 'points': None, 'overflow': False}
    if cap:
        pts = buf[:min(hot + cold, cap)].cpu().numpy()
        info['points'] = np.ascontiguousarray(pts[np.lexsort((pts[:, 1], pts[:, 0]))])
        info['overflow'] = hot + cold > cap
    return out, info


def defect_sites(shape, n, key):
    """n isolated sites of a frame of `shape`, drawn on the host from np.random.default_rng(key): no two within the same-colour 3x3
    footprint of each other (rows and columns both within two), so no site is among another's eight neighbours -- and none in the
    outermost ring of a CFA plane (the frame's first and last two rows and columns): the replicated border makes such a pixel its own
    neighbour, so the detection rule never flags it (only a list repairs it).  Sorted int32 [n][2]."""
    H, W = int(shape[0]), int(shape[1])
    n = int(n)
    if n < 0 or 25 * n > (H - 4) * (W - 4):
        raise ValueError(f"{n} isolated defects do not fit the interior of a {H} x {W} frame (each keeps a 5 x 5 footprint free)")
    rng = np.random.default_rng(int(key))
    taken = np.zeros((H + 4, W + 4), bool)                   # (padded by two: no border cases)
    sites = []
    while len(sites) < n:
        for y, x in zip(rng.integers(2, H - 2, n - len(sites)), rng.integers(2, W - 2, n - len(sites))):
            if not taken[y:y + 5, x:x + 5].any():            # padded (y + 2, x + 2) +- 2
                taken[y + 2, x + 2] = True
                sites.append((y, x))
    pts = np.asarray(sites, np.int32).reshape(-1, 2)
    return np.ascontiguousarray(pts[np.lexsort((pts[:, 1], pts[:, 0]))])


def inject_defects(frame, n, key, level=None, cold_share=0.0, ratio=1.0):
    """For evaluation: (frame with n isolated stuck pixels, sorted truth coordinates int32 [n][2]).  The sites are defect_sites(shape, n,
    key); the first round(cold_share * n) of a keyed shuffle are cold (set to 0), the others hot (set to `level`; default: the frame's
    white level, ratio * 1.0).  A new tensor; plain torch indexing."""
    if not isinstance(frame, torch.Tensor) or frame.dim() != 2:
        raise L.YondHipError("inject_defects: one frame [H][W] as a tensor")
    if not 0.0 <= float(cold_share) <= 1.0:
        raise ValueError(f"cold_share {cold_share!r}: within [0, 1]")
    pts = defect_sites(frame.shape, n, key)
    level = float(ratio) * 1.0 if level is None else float(level)
    order = np.random.default_rng([int(key), 1]).permutation(len(pts))
    n_cold = int(round(float(cold_share) * len(pts)))
    values = np.full(len(pts), level, np.float32)
    values[order[:n_cold]] = 0.0
    out = frame.clone()
    if len(pts):
        idx = torch.from_numpy(pts.astype(np.int64)).to(frame.device)
        out[idx[:, 0], idx[:, 1]] = torch.from_numpy(values).to(frame.device, frame.dtype)
    return out, pts


# ---- the drivers' --bad-pixels / --synth-defects ------------------------------------------------------------------------------------

def bad_pixels_arg(text):
    """argparse type of `--bad-pixels FILE.npy | auto | auto:T`: ('list', path) or ('auto', t)."""
    import argparse
    text = str(text)
    if text == 'auto':
        return ('auto', 6.0)
    if text.startswith('auto:'):
        try:
            t = float(text[5:])
        except ValueError:
            t = float('nan')
        if not (np.isfinite(t) and t > 0):
            raise argparse.ArgumentTypeError(f"auto:T takes a threshold T > 0 in standard deviations, got {text[5:]!r}")
        return ('auto', t)
    if text.endswith('.npy'):
        return ('list', text)
    raise argparse.ArgumentTypeError(f"expected FILE.npy (an int [n][2] array of (row, col)), auto or auto:T, got {text!r}")


def synth_defects_arg(text):
    """argparse type of `--synth-defects N[,LEVEL]`: (n, level or None)."""
    import argparse
    parts = str(text).split(',')
    try:
        n = int(parts[0])
        level = float(parts[1]) if len(parts) == 2 else None
        if len(parts) > 2 or n < 0 or (level is not None and not np.isfinite(level)):
            raise ValueError
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected N or N,LEVEL (a count >= 0 and a finite level in the frame's units), got {text!r}") from None
    return n, level


def bad_pixels_of(pipe, parser=None):
    """None (off, the default), ('list', path) or ('auto', t) from pipe['bad_pixels'] (the runfiles' pipeline key), overridden by the
    parser's --bad-pixels."""
    mode = getattr(parser, 'bad_pixels', None)
    v = (pipe or {}).get('bad_pixels')
    if mode is None and v not in (None, False, 'off'):
        import argparse
        try:
            mode = bad_pixels_arg(v)
        except argparse.ArgumentTypeError as e:
            raise L.YondHipError(f"pipeline.bad_pixels: {e}") from None
    return mode


def load_points(path):
    """The bad-point file of --bad-pixels FILE.npy: int [n][2] (row, col), as a checked int32 array."""
    pts = np.load(str(path), allow_pickle=False)
    if pts.size and (pts.ndim != 2 or pts.shape[1] != 2 or not np.issubdtype(pts.dtype, np.integer)):
        raise L.YondHipError(f"{path}: an integer array [n][2] of (row, col), got shape {pts.shape} of {pts.dtype}")
    return check_points(pts)
