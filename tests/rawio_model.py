"""NumPy statement of the two definitions of include/yond_hip.h R2 / R3 (csrc/rawio.hip): what the kernels, rawio.ingest_host /
emit_host, the loader and the FrameWriter are tested against.  ingest_model is data.py's host expression with the Python scalars
written as the float32 values NumPy makes of them; emit_model is its inverse with one rounding per operation."""
import numpy as np

# (bl, wp) x ratio: the levels of the cameras the runfiles name, a full-range container and a fractional black level
LEVELS = [(64, 1023), (512, 16383), (0, 65535), (256, 4095), (63.5, 1023)]
RATIOS = [1, 2, 3, 10, 100, 200]
GRID = [(bl, wp, r) for bl, wp in LEVELS for r in RATIOS]


def ingest_model(raw, bl, wp, ratio, clip=False):
    with np.errstate(invalid='ignore', over='ignore'):
        x = (raw.astype(np.float32) - np.float32(bl)) * np.float32(ratio) / np.float32(wp - bl)
        return x.clip(0, 1) if clip else x


def _emit_y(x, bl, wp, ratio, undo_gain):
    with np.errstate(invalid='ignore', over='ignore'):
        y = x.astype(np.float32) * np.float32(wp - bl)
        if undo_gain:
            y = y / np.float32(ratio)
        return y, y + np.float32(bl)


def emit_model(x, bl, wp, ratio, undo_gain=False):
    y, yb = _emit_y(x, bl, wp, ratio, undo_gain)
    y = np.where(np.isnan(y), np.float32(0), yb)
    return np.rint(np.clip(y, np.float32(0), np.float32(65535))).astype(np.uint16)


def saturated_model(x, bl, wp, ratio, undo_gain=False):
    """Elements that were NaN or clamped at either end: y + bl is NaN, < 0 or > 65535."""
    _, yb = _emit_y(x, bl, wp, ratio, undo_gain)
    return int(np.count_nonzero(np.isnan(yb) | (yb < 0) | (yb > 65535)))
