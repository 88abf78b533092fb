"""Plain NumPy float64 model of yond_render_srgb (include/yond_hip.h R1): the steps of utils/sidd_utils.py:156-277
(process_sidd_image) and utils/isp_ops.py:171-197 (FastISP) around the project's restatement of cv2's edge-aware demosaic.
Imports nothing from the reference.  tools/gen_golden_isp.py plugs `cv2_cvtcolor` into the reference's cv2 stub, so the
goldens and this model share the demosaic and nothing else.

The codes: code = trunc(max(x, 1e-8) ** (1 / 2.2) * 255).  At a threshold t_k = (k / 255) ** 2.2 the result depends on the last
ulp of NumPy's pow (array and scalar paths differ), so a code is compared only outside the band |x - t_k| <= 2^-48 t_k; inside it
one code of difference is allowed.
"""
import numpy as np

SIDD, FAST = 0, 1
RGB2XYZ = np.array([[0.4124564, 0.3575761, 0.1804375],
                    [0.2126729, 0.7151522, 0.0721750],
                    [0.0193339, 0.1191920, 0.9503041]])
SONY_CCM = np.array([[1.9712269, -0.6789218, -0.29230508],
                     [-0.29104823, 1.748401, -0.45735288],
                     [0.02051281, -0.5380369, 1.5175241]])
FLIPS = {((1, 2), (2, 3)): (False, False), ((2, 1), (3, 2)): (True, False),          # (left-right, up-down)
         ((2, 3), (1, 2)): (False, True), ((3, 2), (2, 1)): (True, True)}
BAND = 2.0 ** -48


def thresholds():
    """t_k = (k / 255) ** 2.2, k = 1 .. 255."""
    return (np.arange(1, 256, dtype=np.float64) / 255.0) ** 2.2


def demosaic(q):
    """q: integers [H][W] on an RGGB mosaic, H and W even -> [H][W][3] RGB integers."""
    q = np.asarray(q).astype(np.int64)
    H, W = q.shape
    p = np.pad(q, 1, mode='reflect')                      # -1 -> 1, H -> H - 2: no repeated edge, CFA parity kept
    c = p[1:-1, 1:-1]
    u, d, l, r = p[:-2, 1:-1], p[2:, 1:-1], p[1:-1, :-2], p[1:-1, 2:]
    diag = (p[:-2, :-2] + p[:-2, 2:] + p[2:, :-2] + p[2:, 2:] + 2) >> 2
    hor, ver = (l + r + 1) >> 1, (u + d + 1) >> 1
    g_rb = np.where(np.abs(l - r) > np.abs(u - d), ver, hor)            # ties go horizontal
    yy, xx = np.mgrid[0:H, 0:W]
    row_r, col_e = (yy & 1) == 0, (xx & 1) == 0
    at_r, at_b = row_r & col_e, ~row_r & ~col_e
    out = np.empty((H, W, 3), np.int64)
    out[..., 0] = np.where(at_r, c, np.where(at_b, diag, np.where(row_r, hor, ver)))
    out[..., 1] = np.where(at_r | at_b, g_rb, c)
    out[..., 2] = np.where(at_b, c, np.where(at_r, diag, np.where(row_r, ver, hor)))
    return out


def cv2_cvtcolor(src, code=None):
    """What tools/gen_golden_isp.py installs as cv2.cvtColor(uint16 Bayer, COLOR_BayerBG2RGB_EA): UNPINNED restatement."""
    return demosaic(src).astype(np.uint16)


def flips_of(bayer_2by2):
    key = tuple(tuple(int(v) for v in row) for row in np.asarray(bayer_2by2).reshape(2, 2).tolist())
    if key not in FLIPS:
        raise ValueError(f"Unknown Bayer pattern {bayer_2by2!r}")
    return FLIPS[key]


def cam2rgb(cst):
    m = np.linalg.inv(np.matmul(np.asarray(cst, np.float64).reshape(3, 3), RGB2XYZ))
    return m / np.sum(m, axis=-1, keepdims=True)


def _site_gains(gains, H, W):
    g = np.empty((H, W), np.float64)
    g[0::2, 0::2], g[0::2, 1::2], g[1::2, 0::2], g[1::2, 1::2] = gains
    return g


def linear(frame, gains, ccm, mode=SIDD, flip_lr=False, flip_ud=False):
    """frame: float32 Bayer [H][W] -> x: float64 [H][W][3] RGB in [0, 1], before the gamma."""
    f = np.asarray(frame, np.float32)
    if flip_lr:
        f = f[:, ::-1]
    if flip_ud:
        f = f[::-1, :]
    H, W = f.shape
    g = _site_gains(gains, H, W)
    if mode == SIDD:
        v = np.clip(np.clip(f, 0, 1).astype(np.float64) * g, 0.0, 1.0)
        q = np.clip(v * 16383.0, 0, 16383).astype(np.int64)
    else:
        v = np.clip((f.astype(np.float64) * g).astype(np.float32), 0, 1)
        q = (v * np.float32(16383)).astype(np.int64)
    dem = demosaic(q)
    d = (dem.astype(np.float32) / np.float32(16383)).astype(np.float64) if mode == SIDD else dem / 16383.0
    m = np.asarray(ccm, np.float64).reshape(3, 3)
    x = np.stack([(d[..., 0] * m[r, 0] + d[..., 1] * m[r, 1]) + d[..., 2] * m[r, 2] for r in range(3)], axis=-1)
    return np.clip(x, 0.0, 1.0)


def codes_of(x):
    return (np.maximum(x, 1e-8) ** (1.0 / 2.2) * 255.0).astype(np.uint8)


def in_band(x):
    """True where x lies within 2^-48 t_k of a threshold t_k: the code there may be either neighbour."""
    t = thresholds()
    k = np.clip(np.searchsorted(t, x), 0, 254)
    near = np.abs(x - t[k]) <= BAND * t[k]
    k2 = np.clip(k - 1, 0, 254)
    return near | (np.abs(x - t[k2]) <= BAND * t[k2])


def render_sidd(frame, bayer_2by2, wb, cst):
    """-> (codes uint8 [H][W][3] RGB, x float64 [H][W][3]).  process_sidd_image returns the codes reversed along the channels (BGR)."""
    lr, ud = flips_of(bayer_2by2)
    wb = np.asarray(wb, np.float64).reshape(-1)
    x = linear(frame, (1 / wb[0], 1 / wb[1], 1 / wb[1], 1 / wb[2]), cam2rgb(cst), SIDD, lr, ud)
    return codes_of(x), x


def unpack4(img4c):
    h, w = img4c.shape[:2]
    raw = np.zeros((2 * h, 2 * w), np.float32)
    raw[0::2, 0::2], raw[0::2, 1::2], raw[1::2, 0::2], raw[1::2, 1::2] = (img4c[..., i] for i in range(4))
    return raw


def fast_isp(img4c, wb=None, ccm=None, gamma=2.2):
    """-> (float64 [H][W][3] RGB in [0, 1], x)."""
    gains = (2.0, 1.0, 1.0, 2.0) if wb is None else (float(wb[0]), 1.0, 1.0, float(wb[2]))
    x = linear(unpack4(np.asarray(img4c, np.float32)), gains, SONY_CCM if ccm is None else ccm, FAST)
    return x ** (1 / gamma), x


def check_codes(got, want, x, what):
    """got == want, or one apart where x is in the band of a threshold."""
    got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    diff = np.abs(got - want)
    band = in_band(x)
    bad = (diff > 1) | ((diff == 1) & ~band)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} codes differ outside the band "
                           f"(max |diff| {int(diff.max())}, first at {tuple(np.argwhere(bad)[0])})")
    return int((diff != 0).sum())
