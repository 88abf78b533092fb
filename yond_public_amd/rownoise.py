"""Row noise (banding) on the device (csrc/rownoise.hip, include/yond_hip.h M5): one offset per sensor row is not Poisson-Gaussian noise
-- the blind estimator's line through (mean, variance) pairs takes it for neither term, the VST does not stabilise it, a denoiser trained
on white noise keeps a structure that is constant along a row, and the low-light protocols multiply it by the digital gain.

`row_denoise` is the reference's utils/isp_algos.py:319-334 for device tensors: the mosaic is split into even and odd sensor rows, each
sequence of row means is smoothed by a 1-D bilateral filter (diameter d = 25, sigma_color = 10, sigma_space = 1 + iso / 200, replicated
border), and `mean - smoothed` is subtracted from the row.  per='plane' is THIS PROJECT'S EXTENSION: one offset per row of a CFA plane
(two per sensor row), the removal that matches the reference's own noise model -- generate_noisy_obs draws its row term as (c, h, 1),
and so does camnoise.py's LAYOUT_PLANAR.  Two launches per frame, no host read between them; there is no CPU fallback.

WHAT IS NOT PINNED.  OpenCV is absent where this was written (oracle/_refimport.py: parity is unpinned at the cv2 boundary), so
cv2.bilateralFilter is restated from its documentation: radius d / 2, weights Gaussian in distance and in value, the result normalised.
To our knowledge OpenCV's float path takes the value weight from an interpolated table, so agreement with a real cv2 is to that table's
accuracy, not to the last bit; and its window is a disc, so on the reference's 1 x n image it also visits the replicated copies of the
row above and below, which reweights the taps by a factor that depends on the distance alone.  Neither could be measured here.

THE METHOD'S LIMITS.  It assumes that the sequence of row means is smooth apart from the noise.  That holds for dark frames, where the
reference uses it; on a scene, content leaks into the offsets.  With the NumPy model on synth_clean(256, 384) * 959 / 2: content alone,
no noise, gives offsets up to 1.06 DN; with K = 1, sigma = 2, sigR = 3 DN the residual row-offset deviation goes from 3.09 to 0.78 DN
(a ratio of 0.24-0.27 over three seeds, 0.33 at sigR = 1); on a 64 x 128 frame of the same generator the content's period is so short
that the method makes banding worse (1.13).  Pixels clipped at the white level carry no row noise and still get the offset; masking
them is out of scope.  The units of sigma_color are the caller's: the reference's 10 is DN of a dark frame.
"""
import numpy as np
import torch

from . import _lib as L

PER = {'row': 0, 'plane': 1}         # YOND_ROWNOISE_ROW / YOND_ROWNOISE_PLANE
MAX_D = 63                           # YOND_ROWNOISE_MAX_D
DEFAULT_ISO = 1600                   # the drivers' ss=auto for an item without an ISO


def _mosaic(t, name):
    t = L.require_cuda(t, name)
    if t.dim() != 2 or t.shape[0] < 2 or t.shape[1] < 2 or t.shape[0] % 2 or t.shape[1] % 2 or t.numel() >= 2 ** 31:
        raise L.YondHipError(f"{name}: one Bayer frame [H][W] with even H and W and fewer than 2^31 pixels, got shape {tuple(t.shape)}")
    return t


def row_sums(raw):
    """float64 [H][2] on the device: sums[y][c] is the sum of raw[y][x] over x % 2 == c.  The same call gives the same bits."""
    raw = _mosaic(raw, "raw")
    H, W = int(raw.shape[0]), int(raw.shape[1])
    sums = torch.empty((H, 2), dtype=torch.float64, device=raw.device)
    with torch.cuda.device(raw.device):
        L.check(L.load().yond_rownoise_sums_f32(L.ptr(raw), H, W, L.ptr(sums), L.stream()), "yond_rownoise_sums_f32")
    return sums


def check_params(sigma_color, sigma_space, d, per):
    """(sigma_color, sigma_space, d, per) as floats / ints / a name, or ValueError."""
    if per not in PER:
        raise ValueError(f"per {per!r}: 'row' (one offset per sensor row, the reference) or 'plane' (one per row of a CFA plane)")
    if isinstance(d, bool) or int(d) != d or int(d) < 1 or int(d) > MAX_D or int(d) % 2 == 0:
        raise ValueError(f"d {d!r}: an odd filter diameter within [1, {MAX_D}]")
    sigma_color, sigma_space = float(sigma_color), float(sigma_space)
    for name, v in (('sigma_color', sigma_color), ('sigma_space', sigma_space)):
        if not (np.isfinite(v) and v > 0):
            raise ValueError(f"{name} {v!r}: finite and > 0")
    return sigma_color, sigma_space, int(d), per


def row_denoise(raw, iso=None, *, sigma_color=10.0, sigma_space=None, d=25, per='row', return_offsets=False):
    """utils/isp_algos.py:319-334 for a device frame [H][W]: a new tensor, `raw` without the row offsets that a bilateral filter along the
    rows of each parity does not explain.  sigma_space=None is the reference's 1 + iso / 200 and needs `iso`; sigma_color is in the
    frame's units.  per='plane' removes one offset per row of a CFA plane.  With return_offsets also the float64 [H][2] offsets that were
    subtracted, still on the device (per='row': both columns equal)."""
    raw = _mosaic(raw, "raw")
    if sigma_space is None:
        if iso is None:
            raise ValueError("row_denoise: sigma_space=None means 1 + iso / 200, which needs iso")
        sigma_space = 1.0 + float(iso) / 200.0
    sigma_color, sigma_space, d, per = check_params(sigma_color, sigma_space, d, per)
    H, W = int(raw.shape[0]), int(raw.shape[1])
    sums = row_sums(raw)
    out = torch.empty_like(raw)
    offsets = torch.empty((H, 2), dtype=torch.float64, device=raw.device) if return_offsets else None
    with torch.cuda.device(raw.device):
        L.check(L.load().yond_rownoise_apply_f32(L.ptr(raw), L.ptr(out), H, W, L.ptr(sums), PER[per], d, sigma_color, sigma_space, L.ptr(offsets),
                                                 L.stream()), "yond_rownoise_apply_f32")
    return (out, offsets) if return_offsets else out


# ---- the drivers' --row-denoise ------------------------------------------------------------------------------------------------------------

def row_denoise_arg(text):
    """argparse type of `--row-denoise [SPEC]`: {'sc': DN at capture, 'ss': float or 'auto', 'd': int, 'per': 'row' | 'plane'}.  SPEC is
    empty or `on` for the defaults sc=10,ss=auto,d=25,per=row, or a comma-separated list of key=value."""
    import argparse
    spec = {'sc': 10.0, 'ss': 'auto', 'd': 25, 'per': 'row'}
    text = '' if text is None or text is True else str(text).strip()
    if text in ('', 'on'):
        return spec
    for part in text.split(','):
        key, eq, val = part.partition('=')
        key, val = key.strip(), val.strip()
        if not eq or key not in spec:
            raise argparse.ArgumentTypeError(f"expected on or sc=..,ss=..|auto,d=..,per=row|plane, got {part!r} in {text!r}")
        try:
            if key == 'per':
                spec[key] = val
            elif key == 'd':
                spec[key] = int(val)
            elif key == 'ss' and val == 'auto':
                spec[key] = 'auto'
            else:
                spec[key] = float(val)
        except ValueError:
            raise argparse.ArgumentTypeError(f"{key}={val!r}: not a number") from None
    try:
        check_params(spec['sc'], 1.0 if spec['ss'] == 'auto' else spec['ss'], spec['d'], spec['per'])
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None
    return spec


def row_denoise_of(pipe, parser=None):
    """None (off, the default) or the spec of row_denoise_arg from pipe['row_denoise'] (the runfiles' pipeline key: True, 'on' or a SPEC),
    overridden by the parser's --row-denoise."""
    spec = getattr(parser, 'row_denoise', None)
    v = (pipe or {}).get('row_denoise')
    if spec is None and v not in (None, False, 'off'):
        import argparse
        try:
            spec = row_denoise_arg(v)
        except argparse.ArgumentTypeError as e:
            raise L.YondHipError(f"pipeline.row_denoise: {e}") from None
    return spec


def frame_units(spec, ratio, wp, bl, iso=None):
    """(sigma_color in the units of the frame the drivers hand on, sigma_space, DN at capture per frame unit): the frame is
    (DN - bl) / (wp - bl) * ratio, so sc DN at capture are sc * ratio / (wp - bl); ss=auto is 1 + iso / 200."""
    span = float(wp) - float(bl)
    ss = 1.0 + float(DEFAULT_ISO if iso is None else iso) / 200.0 if spec['ss'] == 'auto' else float(spec['ss'])
    return float(spec['sc']) * float(ratio) / span, ss, span / float(ratio)


def offsets_report(offsets, dn_per_unit):
    """{'sigma', 'max'}: the RMS and the largest magnitude of the removed offsets in DN at capture -- one tiny reduction, one host read."""
    v = torch.stack([offsets.square().mean().sqrt(), offsets.abs().max()]).cpu().numpy()
    return {'sigma': float(v[0]) * dn_per_unit, 'max': float(v[1]) * dn_per_unit}
