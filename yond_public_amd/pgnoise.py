"""Poisson-Gaussian noise on the GPU: noisy = Poisson(x / beta1) * beta1 + N(0, beta2), the noise model the method rests on
(data_process/yond_datasets.py:720), for a whole batch or frame in one HIP launch (csrc/pgnoise.hip, yond_pg_noise_f32).

Noise is Philox4x32-10 on the device, keyed by (key, slot) per item and counted by the element index: an element's value depends on
its item's parameters, its index and its clean value only.  NumPy's realisation is not reproduced.  The host keeps what is per
item: the (K, sigma) prior of DIV2K_PG_Dataset (sample_pg_params) and the YondPGItem array.  There is no CPU fallback.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from . import img2raw as I

ITEM_DTYPE = np.dtype([('beta1', '<f4'), ('sigma_n', '<f4'), ('exposure', '<f4'), ('key', '<u4'), ('slot', '<u4')])
assert ITEM_DTYPE.itemsize == 20                                # YondPGItem of include/yond_hip.h

# The kernel's thresholds between its regimes (csrc/pgnoise_sampler.h PG_SWITCH_PTRS, PG_SWITCH_NORMAL): inversion below the first,
# PTRS up to the second, a rounded normal above it.
SWITCH_LAMBDAS = (10.0, 8388608.0)

# yond_datasets.py:664-669
NOISE_PRIOR = {'Kmin': -2.5, 'Kmax': 3.5, 'lam': 0.102, 'q': 1 / (2 ** 10), 'wp': 1023, 'bl': 64,
               'sigTLk': 0.85187, 'sigTLb': 0.07991, 'sigTLsig': 0.02921,
               'sigRk': 0.87611, 'sigRb': -2.11455, 'sigRsig': 0.03274,
               'sigGsk': 0.85187, 'sigGsb': 0.67991, 'sigGssig': 0.02921}


def sample_pg_params(rs, prior=NOISE_PRIOR):
    """DIV2K_PG_Dataset.get_noise_params (yond_datasets.py:672-682) on the numpy.random.RandomState `rs`: log K uniform in
    [Kmin, Kmax], log sigma normal around a line in log K whose slope and offset are jittered.  The draws are the reference's, in its
    order, so the result equals the reference's after np.random.seed(s) bit for bit.  K and sigma are in DN of a `scale`-DN range."""
    p = prior
    log_K = rs.uniform(low=p['Kmin'], high=p['Kmax'])
    mu_Gs = (p['sigGsk'] + rs.uniform(-0.2, 0.2)) * log_K + (p['sigGsb'] + rs.uniform(-1, 1))
    log_sigGs = rs.normal(loc=mu_Gs, scale=p['sigGssig'])
    K = np.exp(log_K)
    sigma = np.exp(log_sigGs)
    scale = p['wp'] - p['bl']
    return {'K': K, 'sigma': sigma, 'beta1': K / scale, 'beta2': (sigma / scale) ** 2, 'wp': p['wp'], 'bl': p['bl'], 'scale': scale}


def plan(B, K, sigma, scale, key, slots, exposure=1.0):
    """The YondPGItem array of one launch (host numpy, 20 bytes per item): beta1 = K / scale, sigma_n = sigma / scale.  Every
    parameter is a scalar or a sequence of B values."""
    def per(v, what, dtype=np.float64):
        v = np.asarray(v, dtype)
        if v.ndim and v.shape != (B,):
            raise ValueError(f"{what}: shape {v.shape} for {B} items")
        return np.broadcast_to(v, (B,))
    it = np.zeros(B, ITEM_DTYPE)
    scale = per(scale, 'scale')
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        it['beta1'] = per(K, 'K') / scale
        it['sigma_n'] = per(sigma, 'sigma') / scale
    it['exposure'] = per(exposure, 'exposure')
    it['key'] = per(key, 'key', np.uint32)
    it['slot'] = per(slots, 'slots', np.uint32)
    if not (np.isfinite(it['beta1']).all() and np.isfinite(it['sigma_n']).all() and (it['sigma_n'] >= 0).all()):
        raise ValueError("K / scale must be finite and sigma / scale finite and >= 0")
    if not (np.isfinite(it['exposure']).all() and (it['exposure'] > 0).all()):
        raise ValueError("exposure must be finite and > 0")
    return it


def launch(clean, items, clip=False, out=None):
    """yond_pg_noise_f32 over `clean` ([B][...], device float32, contiguous; any 4-byte-aligned view) for the host item array
    `items` (copied to the device on the current stream).  out: None for a new tensor, `clean` itself for in-place."""
    _lib.require_cuda(clean, "clean")
    B = len(items)
    if clean.numel() == 0 or clean.numel() % B:
        raise ValueError(f"{tuple(clean.shape)} does not hold {B} items of one size")
    out = torch.empty_like(clean) if out is None else _lib.require_cuda(out, "out")
    if out.shape != clean.shape:
        raise ValueError(f"out is {tuple(out.shape)}, clean is {tuple(clean.shape)}")
    d_items = torch.from_numpy(np.ascontiguousarray(items).view(np.uint8)).to(clean.device)
    lib = _lib.load()
    _lib.check(lib.yond_pg_noise_f32(_lib.ptr(clean), _lib.ptr(out), clean.numel() // B, B, C.c_void_p(d_items.data_ptr()),
                                     int(bool(clip)), _lib.stream()), "yond_pg_noise_f32")
    return out


def add_pg_noise(clean, K, sigma, scale, key, slots, exposure=1.0, clip=False, out=None):
    """noisy = (Poisson(max(x, 0) e / beta1) beta1 + sigma_n N(0, 1)) / e + min(x, 0) per element, beta1 = K / scale,
    sigma_n = sigma / scale, e = exposure (1 / ratio for a low-light frame that is scaled back by ratio).

    clean: [B, ...] device float32 with one item per entry of `slots`, or a single frame when `slots` holds one value.
    K, sigma, scale, exposure, key: scalars or per-item sequences; slots: the items' noise slots.  The same (key, slot) gives the
    same noise.  clip clamps the result to [0, 1].  Returns the device tensor (`out` if given; `out=clean` works in place)."""
    slots = np.atleast_1d(np.asarray(slots, np.uint32))
    return launch(clean, plan(len(slots), K, sigma, scale, key, slots, exposure), clip=clip, out=out)


def synth_noise_arg(text):
    """argparse type of `--synth-noise K,SIGMA` (both in DN): (K, sigma) with K > 0 and sigma >= 0."""
    import argparse
    parts = str(text).split(',')
    try:
        K, sigma = (float(v) for v in parts)
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected K,SIGMA (two numbers in DN, e.g. 4,6), got {text!r}") from None
    if not (np.isfinite(K) and np.isfinite(sigma) and K > 0 and sigma >= 0):
        raise argparse.ArgumentTypeError(f"K must be > 0 and SIGMA >= 0 (finite, in DN), got {text!r}")
    return K, sigma


class PGSource(I.Img2RawSource):
    """A directory of sRGB crops as the trainer's batch / eval source of DIV2K_PG_Dataset (yond_datasets.py:661-764): unprocess,
    mosaic and Bayer rotation as Img2RawSource does them (yond_img2raw_f32 with sigma 0 writes hr), then ONE yond_pg_noise_f32 launch
    makes lr from hr with each item's own (K, sigma).  eval_params: the {K, sigma, beta1, beta2, scale, ...} of every evaluation item."""

    def __init__(self, paths, args, device, eval_params):
        super().__init__(paths, args, device, div2k=True)
        self.eval_params = dict(eval_params)

    def _pair(self, patches, pattern, params, key, slots):
        hr, lr, _ = I.launch(self.cache, self.table, patches, pattern=pattern, clip=self.clip)
        add_pg_noise(hr, [q['K'] for q in params], [q['sigma'] for q in params], [q['scale'] for q in params], key, slots,
                     clip=self.clip, out=lr)
        dev = lambda name: torch.tensor([q[name] for q in params], dtype=torch.float32, device=hr.device)
        return {'lr': lr, 'hr': hr, 'sigma': dev('sigma'), 'K': dev('K'), 'beta1': dev('beta1'), 'beta2': dev('beta2')}

    def batch(self, idx, gen, key, slot0):
        """One training batch: metadata and pattern drawn from `gen` as Img2RawSource draws them, (K, sigma) per item from the
        camera-noise prior on a RandomState seeded with (key, slot0), noise (key, slot0 + i).  `sigma` is in DN, as the reference's."""
        metas = [I.sample_meta(gen, self.lock_wb) for _ in idx]
        patterns = [int(torch.randint(4, (1,), generator=gen)) if self.bayer_aug else 0 for _ in idx]
        rs = np.random.RandomState(np.array([key, slot0], np.uint32))
        params = [sample_pg_params(rs) for _ in idx]
        slots = slot0 + np.arange(len(idx))
        p = I.plan(self.cache.offsets(idx), metas, patterns, [0.0] * len(idx), key, slots)
        out = self._pair(p, -1 if self.cache.H == self.cache.W else 0, params, key, slots)
        out.update(pattern=patterns, wb=[I.wb(m) for m in metas])
        return out

    def item(self, idx, sigma=None):
        """Eval item `idx` (batch of one): the reference's metadata after setup_seed(idx), pattern idx % 4, the dataset's fixed
        (K, sigma), noise key idx: every pass gets the same item.  (`sigma`, the AWGN level of the trainer's loop, is not used.)"""
        meta = I.eval_meta(idx, self.lock_wb)
        k = idx % 4 if self.bayer_aug else 0
        p = I.plan(self.cache.offsets([idx]), [meta], [k], [0.0], idx, [0])
        out = self._pair(p, k, [self.eval_params], idx, [0])
        out.update(pattern=k, wb=I.wb(meta), ccm=meta['cam2rgb'].numpy())
        return out
