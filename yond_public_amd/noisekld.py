"""Noise-model fidelity on the device (csrc/noisehist.hip, include/yond_hip.h M3): the KL divergence between the histogram of a real
frame's residual noisy - clean and the histogram of residuals drawn from a noise model on the same clean frame -- the figure the
noise-modelling literature reports (Noise Flow, ELD, PMN), which the reference ships as utils/sidd_utils.py:280-304
(get_histogram / cal_kld).

The kernels count: `residual_hist` bins noisy - clean, `pg_model_hist` bins the Poisson-Gaussian model's residual without storing the
noisy frame (the counts of pgnoise.add_pg_noise followed by residual_hist, integer for integer).  Both split the counts by intensity
band of the clean value and by CFA position; the marginal histogram is their exact integer sum.  The bin edges are built HERE, on the
host, with the reference's own call, and uploaded: np.arange's inner edges are not -R + i * bw to the last bit.  The finish (66 numbers
per histogram) is the reference's NumPy expression in float64, `kld_from_counts`.  There is no CPU fallback for the counting.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import pgnoise as PG

MAX_BINS, MAX_BANDS, MAX_SLOTS = 256, 16, 8448      # YOND_NOISEHIST_MAX_BINS / _MAX_BANDS, and the workgroup's LDS histogram


def kld_edges(half_range=0.1, n_bins=64):
    """cal_kld's bin edges (utils/sidd_utils.py:292-293): n_bins of width 2 R / n_bins on [-R, R] between two catch-all bins that
    reach to +-1000 -- n_bins + 3 edges, n_bins + 2 bins (67 and 66 by default)."""
    R = float(half_range)
    if not (np.isfinite(R) and 0 < R < 1000) or int(n_bins) < 1:
        raise ValueError(f"kld_edges: half_range {half_range!r} must lie in (0, 1000) and n_bins {n_bins!r} be >= 1")
    bw = 2 * R / int(n_bins)
    return np.concatenate(([-1000.0], np.arange(-R, R + 1e-9, bw), [1000.0]), axis=0)


def band_thresholds(bands):
    """The float32 thresholds of `bands`: None or 0 or 1 -> none (one band); an int N -> np.linspace(0, 1, N + 1)[1:-1]; else the
    ascending thresholds themselves.  A pixel's band is the number of thresholds <= its clean value."""
    if bands is None:
        return np.zeros(0, np.float32)
    if isinstance(bands, (int, np.integer)):
        if bands < 0:
            raise ValueError(f"bands {bands!r}: a count >= 0 or a sequence of thresholds")
        return np.linspace(0, 1, int(bands) + 1)[1:-1].astype(np.float32) if bands > 1 else np.zeros(0, np.float32)
    t = np.asarray(bands, np.float32).reshape(-1)
    if not (np.isfinite(t).all() and (np.diff(t) >= 0).all()):
        raise ValueError("band thresholds must be finite and ascending")
    return t


def _edges(edges):
    e = kld_edges() if edges is None else np.ascontiguousarray(edges, np.float64).reshape(-1)
    if e.size < 2 or not np.isfinite(e).all() or not (np.diff(e) >= 0).all():
        raise ValueError("bin edges: at least two finite float64 values, ascending (np.histogram's rule)")
    return e


def _hint(e):
    """The kernel's first guess, floor((r - lo) * inv) + 1: the uniform inner bins of cal_kld's edges.  It never decides a bin."""
    if e.size >= 4 and e[2] > e[1]:
        return float(e[1]), float(1.0 / (e[2] - e[1]))
    return 0.0, 0.0


def _frames(t, name):
    t = L.require_cuda(t, name)
    if t.dim() not in (2, 3) or t.shape[-1] % 2 or t.shape[-2] % 2 or t.numel() == 0:
        raise L.YondHipError(f"{name}: Bayer frame(s) [H][W] or [B][H][W] with even H and W, got shape {tuple(t.shape)}")
    return t


def _launch_args(clean, edges, bands):
    e, t = _edges(edges), band_thresholds(bands)
    nb, nbin = t.size + 1, e.size - 1
    if nbin > MAX_BINS or nb > MAX_BANDS or 4 * nb * nbin > MAX_SLOTS:
        raise L.YondHipError(f"{nb} bands x 4 x {nbin} bins: at most {MAX_BANDS} bands, {MAX_BINS} bins and {MAX_SLOTS} counters in all")
    B = clean.shape[0] if clean.dim() == 3 else 1
    H, W = int(clean.shape[-2]), int(clean.shape[-1])
    d_e = torch.from_numpy(e).to(clean.device)
    d_t = torch.from_numpy(t).to(clean.device) if t.size else None
    counts = torch.empty((B, nb, 4, nbin) if clean.dim() == 3 else (nb, 4, nbin), dtype=torch.int64, device=clean.device)
    return B, H, W, d_e, e.size, d_t, nb, _hint(e), counts


def residual_hist(noisy, clean, edges=None, bands=None):
    """Device counts (int64, [nb][4][n_edges - 1] for a frame [H][W], [B][nb][4][n_edges - 1] for [B][H][W]) of r = noisy - clean, one
    float32 subtraction: index [band of the clean value][CFA position (y & 1) * 2 + (x & 1)][np.histogram's bin of r on `edges`].
    A residual outside the edges, NaN or infinite is counted nowhere.  edges: None for kld_edges(); bands: see band_thresholds."""
    clean, noisy = _frames(clean, "clean"), _frames(noisy, "noisy")
    if noisy.shape != clean.shape or noisy.device != clean.device:
        raise L.YondHipError(f"noisy {tuple(noisy.shape)} on {noisy.device} and clean {tuple(clean.shape)} on {clean.device} do not pair up")
    B, H, W, d_e, ne, d_t, nb, (lo, inv), counts = _launch_args(clean, edges, bands)
    with torch.cuda.device(clean.device):
        L.check(L.load().yond_noise_hist_f32(L.ptr(noisy), L.ptr(clean), B, H, W, L.ptr(d_e), ne, L.ptr(d_t), nb, lo, inv, L.ptr(counts),
                                             L.stream()), "yond_noise_hist_f32")
    return counts


def pg_model_hist(clean, K, sigma, scale, key, edges=None, bands=None, exposure=1.0, clip=False, slots=None):
    """residual_hist(pgnoise.add_pg_noise(clean, K, sigma, scale, key, slots, exposure, clip), clean, edges, bands) in one launch and
    without the noisy frame: the Poisson-Gaussian model's residual histogram on `clean`.  slots: the items' noise slots (default 0 for
    a frame, 0 .. B - 1 for a batch)."""
    clean = _frames(clean, "clean")
    B, H, W, d_e, ne, d_t, nb, (lo, inv), counts = _launch_args(clean, edges, bands)
    slots = np.arange(B, dtype=np.uint32) if slots is None else np.atleast_1d(np.asarray(slots, np.uint32))
    if slots.shape != (B,):
        raise ValueError(f"slots: {slots.shape} for {B} frame(s)")
    items = PG.plan(B, K, sigma, scale, key, slots, exposure)
    d_items = torch.from_numpy(np.ascontiguousarray(items).view(np.uint8)).to(clean.device)
    with torch.cuda.device(clean.device):
        L.check(L.load().yond_pg_noise_hist_f32(L.ptr(clean), B, H, W, C.c_void_p(d_items.data_ptr()), int(bool(clip)), L.ptr(d_e), ne,
                                                L.ptr(d_t), nb, lo, inv, L.ptr(counts), L.stream()), "yond_pg_noise_hist_f32")
    return counts


def _host_counts(c):
    if isinstance(c, torch.Tensor):
        c = c.detach().cpu().numpy()
    return np.asarray(c).astype(np.float64)


def kld_from_counts(p_counts, q_counts, n_p, n_q):
    """(kl_fwd, kl_inv, kl_sym) of two histograms over the same bins, the reference's expression (utils/sidd_utils.py:288, 296-303) in
    NumPy float64: p = counts / n with n the number of data points, uncounted ones included; only bins where both are > 0 take part."""
    p = _host_counts(p_counts).reshape(-1) / n_p
    q = _host_counts(q_counts).reshape(-1) / n_q
    idx = (p > 0) & (q > 0)
    p = p[idx]
    q = q[idx]
    logp = np.log(p)
    logq = np.log(q)
    kl_fwd = np.sum(p * (logp - logq))
    kl_inv = np.sum(q * (logq - logp))
    kl_sym = (kl_fwd + kl_inv) / 2.0
    return float(kl_fwd), float(kl_inv), float(kl_sym)


def _data_counts(data, edges):
    """Marginal device counts of any float32 device tensor: laid out as a two-row Bayer frame (NaN-padded to a multiple of 4: NaN is
    counted nowhere) against a zero clean frame -- x - 0 is x, -0.0 included."""
    data = L.require_cuda(data, "data").reshape(-1)
    n = data.numel()
    if n == 0:
        raise L.YondHipError("data is empty")
    if n % 4:
        data = torch.cat([data, torch.full(((-n) % 4,), float('nan'), dtype=torch.float32, device=data.device)])
    frame = data.view(2, -1)
    return residual_hist(frame, torch.zeros_like(frame), edges).sum(dim=(0, 1)), n


def get_histogram(data, bin_edges=None, left_edge=0.0, right_edge=1.0, n_bins=1000):
    """utils/sidd_utils.py:280-288 for a device tensor: (hist / n, bin_centers) as NumPy float64, the counting on the device."""
    bin_width = (right_edge - left_edge) / n_bins
    if bin_edges is None:
        bin_edges = np.arange(left_edge, right_edge + bin_width, bin_width)
    bin_edges = np.asarray(bin_edges, np.float64)
    counts, n = _data_counts(data, bin_edges)
    return _host_counts(counts) / n, bin_edges[:-1] + (bin_width / 2.0)


def cal_kld(p_data, q_data, left_edge=0.0, right_edge=1.0, n_bins=1000):
    """utils/sidd_utils.py:290-304 for two device tensors: the forward KL divergence of their histograms on kld_edges()."""
    (p, n_p), (q, n_q) = _data_counts(p_data, None), _data_counts(q_data, None)
    return kld_from_counts(p, q, n_p, n_q)[0]


# ---- the drivers' --noise-kld -------------------------------------------------------------------------------------------------------

def noise_kld_arg(text):
    """argparse type of `--noise-kld est | K,SIGMA | cam:<spec>`: ('est',), ('pg', K, sigma) or ('cam', spec)."""
    import argparse
    text = str(text)
    if text == 'est':
        return ('est',)
    if text.startswith('cam:'):
        from .camnoise import camera_noise_arg
        return ('cam', camera_noise_arg(text[4:]))
    try:
        return ('pg',) + tuple(PG.synth_noise_arg(text))
    except argparse.ArgumentTypeError as e:
        raise argparse.ArgumentTypeError(f"expected est, K,SIGMA or cam:<--camera-noise spec>; {e}") from None


def noise_kld_of(pipe, parser=None):
    """(model, half_range, n_bands) from pipe['noise_kld' / 'noise_kld_range' / 'noise_kld_bands'] (the runfiles' pipeline keys), each
    overridden by the parser's --noise-kld / --kld-range / --kld-bands.  model is None when the switch is off."""
    pipe = pipe or {}
    model = getattr(parser, 'noise_kld', None)
    if model is None and pipe.get('noise_kld') not in (None, False, 'off'):
        model = noise_kld_arg(pipe['noise_kld'])
    rng = getattr(parser, 'kld_range', None)
    rng = float(pipe.get('noise_kld_range', 0.1) if rng is None else rng)
    bands = getattr(parser, 'kld_bands', None)
    bands = int(pipe.get('noise_kld_bands', 0) if bands is None else bands)
    if not (np.isfinite(rng) and 0 < rng < 1000):
        raise L.YondHipError(f"noise_kld_range {rng!r}: in (0, 1000)")
    if not 0 <= bands <= MAX_BANDS:
        raise L.YondHipError(f"noise_kld_bands {bands!r}: 0 .. {MAX_BANDS}")
    return model, rng, bands


def kld_report(p_counts, q_counts, n):
    """{'kld', 'kld_cfa' [4], 'kld_bands' [nb]} (forward KL, p the real frame) from two count arrays [nb][4][nbin] of one frame of n
    pixels.  The marginal and the per-CFA / per-band histograms are exact integer sums of the one pass; each is normalised by its own
    pixel count: n / 4 per CFA position (H and W are even); for a band, which is cut on the clean frame and so holds the same pixels on
    both sides, the larger of the two sides' binned counts -- its pixel count unless both sides left pixels unbinned."""
    p, q = _host_counts(p_counts), _host_counts(q_counts)
    out = {'kld': kld_from_counts(p.sum((0, 1)), q.sum((0, 1)), n, n)[0],
           'kld_cfa': [kld_from_counts(p[:, c].sum(0), q[:, c].sum(0), n / 4, n / 4)[0] for c in range(4)]}
    bands = []
    for b in range(p.shape[0]):
        nb_ = max(p[b].sum(), q[b].sum())
        bands.append(kld_from_counts(p[b].sum(0), q[b].sum(0), nb_, nb_)[0] if nb_ > 0 else 0.0)
    out['kld_bands'] = bands
    return out
