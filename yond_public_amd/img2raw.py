"""sRGB crops -> raw training pairs on the GPU: the reference's RGB_Img2Raw_Dataset / DIV2K_Img2Raw_Dataset item
(data_process/yond_datasets.py:277-334, :483-548) for a whole batch in one HIP launch (csrc/img2raw.hip, yond_img2raw_f32).

The host keeps what is per patch or per level, never per pixel:
  - the metadata sampler (data_process/unprocess.py:7-59): rgb2cam, rgb_gain, red / blue gains drawn from a torch.Generator in the
    reference's call order, so that an eval item's metadata equals the reference's after setup_seed(idx) bit for bit;
  - the transfer curve gamma_expansion(inverse_smoothstep(level / divisor)) (unprocess.py:80-95) as a table of 256 or 65536 levels,
    evaluated in float32 with torch as the reference evaluates it per pixel;
  - a device crop cache filled lazily from the .npy files (one copy per crop, the first time a batch needs it);
  - the batch planner: indices -> YondImg2RawPatch array (crop offset, CCM, gains, pattern, sigma, noise key / slot).
Noise is Philox4x32-10 + Box-Muller on the device, keyed by (key, slot): the reference's NumPy realisation is not reproduced.
There is no CPU fallback: a CPU device raises.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib

# unprocess.py:11-23, 32-34 (Brooks et al., "Unprocessing Images for Learned Raw Denoising", CVPR 2019)
XYZ2CAMS = [[[1.0234, -0.2969, -0.2266], [-0.5625, 1.6328, -0.0469], [-0.0703, 0.2188, 0.6406]],
            [[0.4913, -0.0541, -0.0202], [-0.613, 1.3513, 0.2906], [-0.1564, 0.2151, 0.7183]],
            [[0.838, -0.263, -0.0639], [-0.2887, 1.0725, 0.2496], [-0.0627, 0.1427, 0.5438]],
            [[0.6596, -0.2079, -0.0562], [-0.4782, 1.3016, 0.1933], [-0.097, 0.1581, 0.5181]]]
RGB2XYZ = [[0.4124564, 0.3575761, 0.1804375], [0.2126729, 0.7151522, 0.0721750], [0.0193339, 0.1191920, 0.9503041]]

PATCH_DTYPE = np.dtype([('rgb2cam', '<f4', 9), ('gain', '<f4', 3), ('sigma', '<f4'), ('pattern', '<i4'), ('key', '<u4'),
                        ('slot', '<u4'), ('offset', '<i8')], align=True)      # YondImg2RawPatch of include/yond_hip.h
assert PATCH_DTYPE.itemsize == 72


# -- metadata ------------------------------------------------------------------------------------------------------------------
def random_gains(gen=None):
    """unprocess.py:50-59 on `gen`: rand(1), the normal, red, blue, in that order.  (rgb_gain, red, blue), (1,) float32 tensors."""
    bright = torch.rand(1, generator=gen) < 0.9
    n = torch.normal(torch.tensor([0.8]), torch.tensor([0.1]), generator=gen)
    rgb_gain = 1.0 / n if bright else 0.2 / n
    red = torch.empty(1).uniform_(1.4, 2.5, generator=gen)
    blue = torch.empty(1).uniform_(1.5, 2.4, generator=gen)
    return rgb_gain, red, blue


def sample_meta(gen, lock_wb=False):
    """unprocess.py:180-183 on `gen`: rgb2cam (random_ccm, :7-47), then the gains (random_gains, :50-59) unless lock_wb is a
    [rgb_gain, red, blue] triple.  The draws are the reference's, in its order: 4 weights, rand(1), normal, red, blue.
    Returns {'rgb2cam': (3, 3), 'cam2rgb': (3, 3), 'rgb_gain', 'red', 'blue': (1,)} float32 tensors."""
    w = torch.empty(len(XYZ2CAMS), 1, 1).uniform_(1e-8, 1e8, generator=gen)
    xyz2cam = torch.sum(torch.tensor(XYZ2CAMS) * w, dim=0) / torch.sum(w, dim=0)
    rgb2cam = torch.mm(xyz2cam, torch.tensor(RGB2XYZ))
    rgb2cam = rgb2cam / torch.sum(rgb2cam, dim=-1, keepdim=True)
    if lock_wb is False or lock_wb is None:
        rgb_gain, red, blue = random_gains(gen)
    else:
        rgb_gain, red, blue = torch.tensor(np.asarray(lock_wb, np.float32)).reshape(3, 1)
    return {'rgb2cam': rgb2cam, 'cam2rgb': torch.inverse(rgb2cam), 'rgb_gain': rgb_gain, 'red': red, 'blue': blue}


def eval_meta(idx, lock_wb=False):
    """The metadata of eval item `idx`: the reference calls setup_seed(idx) right before unprocess (yond_datasets.py:289)."""
    return sample_meta(torch.Generator().manual_seed(int(idx)), lock_wb)


def gains(meta):
    """safe_invert_gains' per-channel gains (unprocess.py:112): [1/red, 1, 1/blue] / rgb_gain in float32."""
    return (torch.stack((1.0 / meta['red'], torch.tensor([1.0]), 1.0 / meta['blue'])) / meta['rgb_gain']).reshape(3)


def wb(meta):
    """data['wb'] of the reference item (yond_datasets.py:298)."""
    return np.array([meta['red'].item(), 1., meta['blue'].item()])


def train_streams(epoch, rank, seed=1997):
    """(torch.Generator, noise key) of one (epoch, rank): every rank draws its own metadata and noise."""
    s = np.random.SeedSequence([int(epoch), int(rank), int(seed)]).generate_state(3, np.uint32)
    return torch.Generator().manual_seed(int(s[0]) | (int(s[1]) << 32)), int(s[2])


def sample_item(gen, sigma_min, sigma_max, lock_wb=False, bayer_aug=True):
    """One training item's draws: the metadata, the pattern (randint(4); 0 under no_bayeraug), sigma log-uniform in
    [sigma_min, sigma_max] / 255 (yond_datasets.py:293-318)."""
    meta = sample_meta(gen, lock_wb)
    pattern = int(torch.randint(4, (1,), generator=gen)) if bayer_aug else 0
    lo, hi = np.log(sigma_min), np.log(sigma_max)
    sigma = float(np.exp(float(torch.rand(1, dtype=torch.float64, generator=gen)) * (hi - lo) + lo) / 255.)
    return meta, pattern, sigma


# -- transfer curve -----------------------------------------------------------------------------------------------------------
def curve_host(dtype, divisor):
    """gamma_expansion(inverse_smoothstep(level / divisor)) for every level of `dtype` (unprocess.py:80-95), float32."""
    n = 256 if np.dtype(dtype) == np.uint8 else 65536
    x = torch.arange(n, dtype=torch.float32) / float(divisor)
    x = torch.clamp(x, min=0.0, max=1.0)
    x = 0.5 - torch.sin(torch.asin(1.0 - 2.0 * x) / 3.0)
    return torch.clamp(x, min=1e-8) ** 2.2


_CURVES = {}


def curve(dtype, divisor, device):
    key = (np.dtype(dtype).str, float(divisor), str(device))
    if key not in _CURVES:
        _CURVES[key] = curve_host(dtype, divisor).to(device)
    return _CURVES[key]


# -- crop files ---------------------------------------------------------------------------------------------------------------
def npy_header(path):
    """(shape, dtype) of a .npy file without reading its data."""
    a = np.load(path, mmap_mode='r')
    return tuple(a.shape), a.dtype


def is_srgb(shape, dtype):
    return len(shape) == 3 and shape[-1] == 3 and np.dtype(dtype) in (np.uint8, np.uint16)


def crop_kind(paths):
    """'srgb' if every file is an (H, W, 3) uint8 / uint16 crop, 'packed' if none is, None for no files; a mixed directory raises
    (naming a file of each kind)."""
    srgb, other = [], []
    for p in paths:
        (srgb if is_srgb(*npy_header(p)) else other).append(p)
    if srgb and other:
        raise ValueError(f"{os.path.dirname(srgb[0])} mixes sRGB crops (H, W, 3) uint8/uint16 ({len(srgb)} files, e.g. "
                         f"{os.path.basename(srgb[0])}) with packed raw patches ({len(other)} files, e.g. {os.path.basename(other[0])}): "
                         "a dataset directory holds one kind")
    return 'srgb' if srgb else ('packed' if other else None)


class CropCache:
    """The crops of one directory in one device buffer ([n][H][W][3] of their dtype), each filled the first time it is needed."""

    def __init__(self, paths, device):
        if torch.device(device).type != 'cuda':
            raise _lib.YondHipError("the img2raw crop cache lives on a ROCm device (the HIP path has no CPU fallback)")
        self.paths = list(paths)
        shapes = {npy_header(p) for p in self.paths}
        if len(shapes) != 1:
            raise ValueError(f"sRGB crops of one dataset must share shape and dtype (one batch is one launch), found "
                             f"{sorted((s, str(d)) for s, d in shapes)}")
        (self.shape, self.dtype), = shapes
        if not is_srgb(self.shape, self.dtype) or self.shape[0] % 2 or self.shape[1] % 2:
            raise ValueError(f"expected (H, W, 3) uint8 / uint16 crops with H and W even, got {self.shape} {self.dtype}")
        self.H, self.W = self.shape[:2]
        tdt = torch.uint8 if self.dtype == np.uint8 else torch.int16      # uint16 bits travel as int16
        self.buf = torch.empty((len(self.paths), self.H, self.W, 3), dtype=tdt, device=device)
        self.filled = np.zeros(len(self.paths), bool)
        self.per = self.H * self.W * 3

    def offsets(self, idx):
        """Element offsets of crops `idx` in `buf`, loading the ones not there yet."""
        idx = np.asarray(idx, np.int64)
        for i in np.unique(idx[~self.filled[idx]]):
            a = np.ascontiguousarray(np.load(self.paths[i]))
            if a.shape != self.shape or a.dtype != self.dtype:
                raise ValueError(f"{self.paths[i]}: {a.shape} {a.dtype}, the directory's crops are {self.shape} {self.dtype}")
            self.buf[i].copy_(torch.from_numpy(a.view(np.uint8 if a.dtype == np.uint8 else np.int16)))
            self.filled[i] = True
        return idx * self.per


# -- planner + launch ---------------------------------------------------------------------------------------------------------
def plan(offsets, metas, patterns, sigmas, key, slots):
    """The YondImg2RawPatch array of one batch (host numpy, 72 bytes per patch)."""
    p = np.zeros(len(offsets), PATCH_DTYPE)
    p['rgb2cam'] = np.stack([m['rgb2cam'].numpy().reshape(9) for m in metas])
    p['gain'] = np.stack([gains(m).numpy() for m in metas])
    p['sigma'] = np.asarray(sigmas, np.float32)
    p['pattern'] = np.asarray(patterns, np.int32)
    p['key'] = np.uint32(key)
    p['slot'] = np.asarray(slots, np.uint32)
    p['offset'] = np.asarray(offsets, np.int64)
    return p


def launch(cache, table, patches, pattern=-1, clip=True, hr=None, lr=None, sigma=None):
    """yond_img2raw_f32 over `cache` for the host patch array `patches` (copied to the device on the current stream).
    pattern: -1 = each patch's own (square crops), 0..3 = the same rotation for all.  Returns (hr, lr, sigma) on the device:
    [B][4][h'][w'], [B][4][h'][w'], [B]."""
    dev = cache.buf.device
    B = len(patches)
    k = int(patches['pattern'][0]) if pattern < 0 else int(pattern)
    ho, wo = (cache.W // 2, cache.H // 2) if k & 1 else (cache.H // 2, cache.W // 2)
    if pattern < 0 and cache.H != cache.W:
        raise ValueError(f"per-patch Bayer rotations need square crops, these are {cache.H} x {cache.W}")
    pd = torch.from_numpy(patches.view(np.uint8)).to(dev)
    hr = torch.empty((B, 4, ho, wo), dtype=torch.float32, device=dev) if hr is None else hr
    lr = torch.empty_like(hr) if lr is None else lr
    sigma = torch.empty(B, dtype=torch.float32, device=dev) if sigma is None else sigma
    for t in (hr, lr, sigma):
        _lib.require_cuda(t)
    assert hr.shape == lr.shape == (B, 4, ho, wo) and sigma.numel() == B
    lib = _lib.load()
    _lib.check(lib.yond_img2raw_f32(C.c_void_p(cache.buf.data_ptr()), cache.buf.numel(), 0 if cache.dtype == np.uint8 else 1,
                                    cache.H, cache.W, _lib.ptr(table), C.c_void_p(pd.data_ptr()), B, int(pattern), int(bool(clip)),
                                    _lib.ptr(hr), _lib.ptr(lr), _lib.ptr(sigma), _lib.stream()), "yond_img2raw_f32")
    return hr, lr, sigma


class Img2RawSource:
    """A directory of sRGB crops as the trainer's batch / eval source (the device path beside RGB_Img2Raw_Dataset, whose host
    items stay packed-raw only).  divisor: 255 for uint8 and 65535 for uint16 (RGB_Img2Raw_Dataset, :283), 255 always for DIV2K."""

    def __init__(self, paths, args, device, div2k=False):
        self.args = dict(args)
        self.cache = CropCache(paths, device)
        self.divisor = 255. if (div2k or self.cache.dtype == np.uint8) else 65535.
        self.table = curve(self.cache.dtype, self.divisor, device)
        self.lock_wb = self.args.get('lock_wb', False)
        self.clip = bool(self.args.get('clip', False))
        self.bayer_aug = div2k or 'no_bayeraug' not in self.args.get('command', '')
        if self.args.get('mode') == 'train' and self.bayer_aug and self.cache.H != self.cache.W:
            raise ValueError(f"{os.path.dirname(self.cache.paths[0])}: {self.cache.H} x {self.cache.W} crops with Bayer-pattern "
                             "augmentation: an odd rotation changes a non-square crop's shape, so a batch could not be stacked "
                             "(the reference's collate fails on it too); use square crops or `command: no_bayeraug`")

    def __len__(self):
        return len(self.cache.paths)

    def batch(self, idx, gen, key, slot0):
        """One training batch: items `idx` drawn from `gen`, noise (key, slot0 + i).  Returns the trainer's batch dict with
        device lr / hr / sigma."""
        draws = [sample_item(gen, self.args['sigma_min'], self.args['sigma_max'], self.lock_wb, self.bayer_aug) for _ in idx]
        metas, patterns, sigmas = zip(*draws)
        p = plan(self.cache.offsets(idx), metas, patterns, sigmas, key, slot0 + np.arange(len(idx)))
        hr, lr, sigma = launch(self.cache, self.table, p, pattern=-1 if self.cache.H == self.cache.W else 0, clip=self.clip)
        return {'lr': lr, 'hr': hr, 'sigma': sigma, 'pattern': list(patterns), 'wb': [wb(m) for m in metas]}

    def item(self, idx, sigma):
        """Eval item `idx` (batch of one): the reference's metadata after setup_seed(idx), pattern idx % 4 (0 under no_bayeraug),
        the fixed sigma, noise key idx: every pass gets the same item."""
        meta = eval_meta(idx, self.lock_wb)
        k = idx % 4 if self.bayer_aug else 0
        p = plan(self.cache.offsets([idx]), [meta], [k], [sigma], idx, [0])
        hr, lr, s = launch(self.cache, self.table, p, pattern=k, clip=self.clip)
        return {'lr': lr, 'hr': hr, 'sigma': s, 'pattern': k, 'wb': wb(meta), 'ccm': meta['cam2rgb'].numpy()}
