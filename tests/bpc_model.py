"""The specification of the defective-pixel kernels (include/yond_hip.h M4) in NumPy float64.

The reference's repair (utils/isp_ops.py:152-160 repair_bad_pixels) is `cv2.medianBlur(plane, 3)` on each of bayer2rggb's four planes,
written back at the listed points.  OpenCV is not among this project's dependencies, so the median here is a RESTATEMENT of
cv2.medianBlur(., 3) -- the median of the 3x3 window with BORDER_REPLICATE -- in mosaic coordinates, as oracle/_refimport.py restates
cv2.blur: the same-colour neighbourhood of (y, x) is (cy(y + 2 dy), cx(x + 2 dx)), dy, dx in {-1, 0, 1}, with cy clamping to
[y & 1, H - 2 + (y & 1)] and cx likewise.  A median of nine float32 values is a selection: no rounding is involved.

The blind detection rule is this project's extension (no reference): every operation below is one NumPy float64 operation, so each
is rounded on its own, as the kernel's are (no contraction into an FMA: see bpc_flag in csrc/bpc.hip).
"""
import numpy as np


def _clamped(n, d):
    """Indices cy(i + 2 d) of i = 0 .. n - 1."""
    i = np.arange(n)
    p = i & 1
    return np.minimum(np.maximum(i + 2 * d, p), n - 2 + p)


def neighbourhood(frame):
    """[9][H][W]: the same-colour 3x3 neighbourhood of every pixel, index 3 * (dy + 1) + (dx + 1); [4] is the frame itself."""
    frame = np.asarray(frame)
    H, W = frame.shape
    assert H >= 2 and W >= 2 and H % 2 == 0 and W % 2 == 0, (H, W)
    return np.stack([frame[_clamped(H, dy)][:, _clamped(W, dx)] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])


def median9(frame):
    """m(y, x): the median of the nine, centre included (dtype of the frame: a selection)."""
    return np.sort(neighbourhood(frame), axis=0)[4]


def in_frame(points, shape):
    """The rows of `points` ([n][2] (row, col)) that lie inside a frame of `shape`."""
    pts = np.asarray(points, np.int64).reshape(-1, 2)
    ok = (pts[:, 0] >= 0) & (pts[:, 0] < shape[0]) & (pts[:, 1] >= 0) & (pts[:, 1] < shape[1])
    return pts[ok]


def repair_list(frame, points):
    """List mode: the input with m written at every listed point inside the frame; m is taken from the INPUT frame."""
    frame = np.asarray(frame)
    out = frame.copy()
    pts = in_frame(points, frame.shape)
    if len(pts):
        m = median9(frame)
        out[pts[:, 0], pts[:, 1]] = m[pts[:, 0], pts[:, 1]]
    return out


def detect(frame, beta1, beta2, t=6.0):
    """(hot, cold): boolean maps of the rule, float64 from the float32 pixels."""
    nb = neighbourhood(np.asarray(frame, np.float32))
    c = nb[4].astype(np.float64)
    others = nb[[0, 1, 2, 3, 5, 6, 7, 8]]
    hi, lo = others.max(axis=0).astype(np.float64), others.min(axis=0).astype(np.float64)     # (max / min of float32 values: selections)
    beta1, beta2, t2 = np.float64(beta1), np.float64(beta2), np.float64(t) * np.float64(t)
    with np.errstate(invalid='ignore', over='ignore'):
        d = c - hi
        hot = (c > hi) & (d * d > t2 * (beta1 * np.maximum(hi, 0.0) + beta2))
        d = lo - c
        cold = (c < lo) & (d * d > t2 * (beta1 * np.maximum(lo, 0.0) + beta2))
    return hot, cold


def detect_and_repair(frame, beta1, beta2, t=6.0):
    """Auto mode: (out, {'hot', 'cold', 'points'}) -- flagged pixels get m, all others are copied; points sorted by (row, col)."""
    frame = np.asarray(frame, np.float32)
    hot, cold = detect(frame, beta1, beta2, t)
    flagged = hot | cold
    out = np.where(flagged, median9(frame), frame)
    return out, {'hot': int(hot.sum()), 'cold': int(cold.sum()), 'points': np.argwhere(flagged).astype(np.int32)}


def certain_bound(clean_max, beta1, beta2, t=6.0):
    """A value above M + t * sqrt(beta1 * M + beta2), M the maximum of the undisturbed frame, is flagged wherever its eight neighbours
    are undisturbed pixels: hi <= M, and v - hi - t sqrt(beta1 max(hi, 0) + beta2) does not grow with hi (beta1 >= 0).  That leaves out
    the outermost ring of each CFA plane (rows and columns 0, 1, n - 2, n - 1 of the mosaic): with the replicated border such a pixel is
    among its own neighbours, hi >= c, and the rule never flags it."""
    M = float(clean_max)
    return M + float(t) * np.sqrt(beta1 * max(M, 0.0) + beta2)
