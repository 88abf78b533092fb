"""Whole clean raw frames -> raw training pairs on the GPU: the reference's SID_Raw_Dataset item
(data_process/yond_datasets.py:46-212) for a whole batch in one HIP launch (csrc/rawcrop.hip, yond_rawcrop_f32).

The frames of a dataset stay resident on the device as they are stored (uint16, or float32 DN); a training patch is cut from them
per element: DN normalisation, Bayer-pattern rotation, packing, [0, 1] clip, square-root ("VST") augmentation of the ground truth,
the crop, brightness / white-balance jitter and AWGN.  The host keeps what is per frame, never per pixel:
  - the draws of one item (`sample_item`): pattern, vst_aug, crop origins, the gain coin, random_gains() (unprocess.py:50-59), sigma,
    in the reference's order.  Training draws come from the per-(epoch, rank) torch.Generator of img2raw.train_streams; the
    reference draws them from NumPy's and torch's global generators, whose stream a test can replay through `sample_item`;
  - the batch planner: frames x crop_per_image -> YondRawCropPatch array, every crop checked against its rotated frame.
Noise is Philox4x32-10 + Box-Muller on the device, keyed by (key, slot): the reference's NumPy realisation is not reproduced.
There is no CPU fallback: a CPU device raises.

Two departures from the reference, both on purpose:
  - it draws an evaluation item's vst_aug from the global generator BEFORE setup_seed(idx) (:168, :178), so its evaluation items
    differ from pass to pass; here vst_aug of evaluation item idx is (idx // 4) % 2, next to pattern idx % 4;
  - it writes the jittered white balance back into its info entry (:190-191), so a frame's `wb` drifts from epoch to epoch; here
    the file's `wb` is the base of every draw.
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib
from .img2raw import npy_header, random_gains

PATCH_DTYPE = np.dtype([('frame', '<i8'), ('y0', '<i4'), ('x0', '<i4'), ('pattern', '<i4'), ('vst_aug', '<i4'), ('rgb_gain', '<f4'),
                        ('gain0', '<f8'), ('gain2', '<f8'), ('sigma', '<f4'), ('key', '<u4'), ('slot', '<u4')],
                       align=True)                                      # YondRawCropPatch of include/yond_hip.h
assert PATCH_DTYPE.itemsize == 64 and PATCH_DTYPE.fields['gain0'][1] == 32


# -- draws ---------------------------------------------------------------------------------------------------------------------
class TorchDraws:
    """The integer / uniform draws of `sample_item` on a torch.Generator.  Anything with `integers(n, size=None)`, `random()` and
    a torch generator `gen` (None = torch's global one) can stand in: tests replay the reference's NumPy stream that way."""

    def __init__(self, gen):
        self.gen = gen

    def integers(self, n, size=None):
        t = torch.randint(int(n), (1 if size is None else int(size),), generator=self.gen)
        return int(t) if size is None else t.numpy()

    def random(self):
        return float(torch.rand(1, dtype=torch.float64, generator=self.gen))


def apply_gains(draw, wb, gains):
    """The multipliers of yond_datasets.py:184-191 for one frame: float32 rgb_gain, float64 wb[0] / red and wb[2] / blue (a float64
    white balance over a float32 gain), and the item's `wb`."""
    wb = np.asarray(wb, np.float64)
    if gains is None:
        return dict(draw, rgb_gain=np.float32(1), gain0=1.0, gain2=1.0, wb=wb.copy(), gains=None)
    rgb_gain, red, blue = (g.numpy() for g in gains)
    gain0, gain2 = float((wb[0] / red)[0]), float((wb[2] / blue)[0])
    return dict(draw, rgb_gain=np.float32(rgb_gain[0]), gain0=gain0, gain2=gain2, wb=np.array([gain0, wb[1], gain2]),
                gains=np.array([rgb_gain[0], red[0], blue[0]], np.float32))


def sample_item(gen, h, w, patch_size, crop_per_image, croptype, sigma_min, sigma_max, lock_wb=False, wb=(1., 1., 1.)):
    """One training item's draws (all crop_per_image patches of one frame share them but the origins), in the reference's order
    (yond_datasets.py:164-198): pattern, vst_aug, [the unused flip modes of :115], the crop origins on the UNROTATED packed (h, w)
    -- 'non-overlapped': one grid offset, cells in row-major order (:119-129); anything else: independent origins (:131-138) --
    swapped for an odd pattern (:174-175), the gain coin unless lock_wb, random_gains(), sigma log-uniform in
    [sigma_min, sigma_max] / 255.  gen: a torch.Generator or a TorchDraws-like object.  check_crops() says beforehand whether
    the patches fit; plan() refuses any that do not."""
    d = gen if hasattr(gen, 'integers') else TorchDraws(gen)
    ps, n = int(patch_size), int(crop_per_image)
    pattern = d.integers(4)
    vst_aug = d.integers(2)
    d.integers(8, size=n)                                  # self.aug: drawn and unused by the reference too (:115, :148)
    if croptype == 'non-overlapped':
        nh, nw = h // ps, w // ps
        hs, ws = d.integers(h - nh * ps + 1), d.integers(w - nw * ps + 1)
        ys = [hs + (i // nw) * ps for i in range(n)]
        xs = [ws + (i % nw) * ps for i in range(n)]
    else:
        ys, xs = [], []
        for _ in range(n):
            ys.append(d.integers(h - ps + 1))
            xs.append(d.integers(w - ps + 1))
    if pattern % 2:
        ys, xs = xs, ys
    gains = None
    if lock_wb is False and d.integers(2):
        gains = random_gains(d.gen)
    lo, hi = np.log(sigma_min), np.log(sigma_max)
    sigma = float(np.exp(d.random() * (hi - lo) + lo) / 255.)
    return apply_gains(dict(pattern=int(pattern), vst_aug=int(vst_aug), y0=[int(v) for v in ys], x0=[int(v) for v in xs], sigma=sigma),
                       wb, gains)


def eval_draws(idx, wb=(1., 1., 1.), lock_wb=False):
    """The draws of evaluation item `idx` (the whole frame, no crop): pattern idx % 4; after setup_seed(idx) the gain coin comes
    from NumPy's legacy generator and the gains from torch's generator seeded with idx, so the item's `wb` equals the reference's
    bit for bit.  The reference draws vst_aug BEFORE it seeds, so its evaluation items are not reproducible: here vst_aug is
    (idx // 4) % 2 -- every (pattern, vst_aug) pair appears among eight consecutive items and every pass sees the same item."""
    idx = int(idx)
    gains = None
    if lock_wb is False and np.random.RandomState(idx).randint(2):
        gains = random_gains(torch.Generator().manual_seed(idx))
    return apply_gains(dict(pattern=idx % 4, vst_aug=(idx // 4) % 2, y0=[0], x0=[0], sigma=None), wb, gains)


# -- frames --------------------------------------------------------------------------------------------------------------------
def frame_shape(paths, headers=None):
    """(H, W, dtype) shared by every frame file; a ValueError naming the files otherwise.  headers: [(shape, dtype)] when the frames
    are arrays, not files."""
    headers = [npy_header(p) for p in paths] if headers is None else headers
    kinds = {}
    for p, (shape, dtype) in zip(paths, headers):
        kinds.setdefault((tuple(shape), np.dtype(dtype).str), []).append(os.path.basename(str(p)))
    if len(kinds) != 1:
        raise ValueError("the raw frames of one dataset must share shape and dtype (one batch is one launch), found "
                         + "; ".join(f"{s} {np.dtype(d).name}: {', '.join(f[:3])}{' ...' if len(f) > 3 else ''}"
                                     for (s, d), f in sorted(kinds.items())))
    (shape, dtype), names = next(iter(kinds.items()))
    dtype = np.dtype(dtype)
    if len(shape) != 2 or dtype not in (np.dtype(np.uint16), np.dtype(np.float32)):
        raise ValueError(f"expected (H, W) Bayer frames of uint16 or float32 DN, got {shape} {dtype.name} ({', '.join(names[:3])})")
    if shape[0] % 2 or shape[1] % 2 or min(shape) < 2:
        raise ValueError(f"a Bayer frame packs to (H/2, W/2, 4): H and W must be even, got {shape[0]} x {shape[1]} ({', '.join(names[:3])})")
    return shape[0], shape[1], dtype


class FrameCache:
    """The frames of one dataset in one device buffer ([n][H][W] of their dtype), each filled the first time it is needed.
    frames: the arrays themselves (synthetic data); `paths` then only names them."""

    def __init__(self, paths, device, frames=None):
        if torch.device(device).type != 'cuda':
            raise _lib.YondHipError("the raw frame cache lives on a ROCm device (the HIP path has no CPU fallback)")
        self.paths, self.frames = list(paths), frames
        self.H, self.W, self.dtype = frame_shape(self.paths, None if frames is None else [(f.shape, f.dtype) for f in frames])
        tdt = torch.int16 if self.dtype == np.uint16 else torch.float32      # uint16 bits travel as int16
        self.buf = torch.empty((len(self.paths), self.H, self.W), dtype=tdt, device=device)
        self.filled = np.zeros(len(self.paths), bool)
        self.per = self.H * self.W

    def offsets(self, idx):
        """Element offsets of frames `idx` in `buf`, loading the ones not there yet."""
        idx = np.asarray(idx, np.int64)
        for i in np.unique(idx[~self.filled[idx]]):
            a = np.ascontiguousarray(np.load(self.paths[i]) if self.frames is None else self.frames[i])
            if a.shape != (self.H, self.W) or a.dtype != self.dtype:
                raise ValueError(f"{self.paths[i]}: {a.shape} {a.dtype}, the dataset's frames are {(self.H, self.W)} {self.dtype}")
            self.buf[i].copy_(torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a))
            self.filled[i] = True
        return idx * self.per


# -- planner + launch ----------------------------------------------------------------------------------------------------------
def plan(offsets, items, H, W, ps, key, slots):
    """The YondRawCropPatch array of one batch (host numpy, 64 bytes per patch): frame offsets[i] with the draws items[i] gives
    len(items[i]['y0']) patches.  A crop outside its rotated frame raises here, before any launch."""
    n = sum(len(it['y0']) for it in items)
    p = np.zeros(n, PATCH_DTYPE)
    slots = np.broadcast_to(np.asarray(slots, np.uint32), (n,))
    b = 0
    for off, it in zip(offsets, items):
        k = int(it['pattern'])
        if not 0 <= k <= 3:
            raise ValueError(f"pattern {k} is not a number of quarter turns 0..3")
        ho, wo = (W // 2, H // 2) if k & 1 else (H // 2, W // 2)
        for y0, x0 in zip(it['y0'], it['x0']):
            if y0 < 0 or x0 < 0 or y0 + ps > ho or x0 + ps > wo or ps < 1:
                raise ValueError(f"crop ({y0}, {x0}) + {ps} leaves the {ho} x {wo} packed frame (pattern {k} of {H} x {W})")
            p[b] = (off, y0, x0, k, int(bool(it['vst_aug'])), it['rgb_gain'], it['gain0'], it['gain2'], it['sigma'], 0, 0)
            b += 1
    p['key'] = np.uint32(key)
    p['slot'] = slots
    return p


def launch(cache, patches, ps, bl, wp, clip=True, hr=None, lr=None, sigma=None):
    """yond_rawcrop_f32 over `cache` for the host patch array `patches` (checked by the library on the host, handed to the kernel
    by value: free again on return).  Returns (hr, lr, sigma) on the device: [B][4][ps][ps], [B][4][ps][ps], [B]."""
    dev = cache.buf.device
    B, ps = len(patches), int(ps)
    patches = np.ascontiguousarray(patches, PATCH_DTYPE)
    hr = torch.empty((B, 4, ps, ps), dtype=torch.float32, device=dev) if hr is None else hr
    lr = torch.empty_like(hr) if lr is None else lr
    sigma = torch.empty(B, dtype=torch.float32, device=dev) if sigma is None else sigma
    for t in (hr, lr, sigma):
        _lib.require_cuda(t)
    assert hr.shape == lr.shape == (B, 4, ps, ps) and sigma.numel() == B
    lib = _lib.load()
    _lib.check(lib.yond_rawcrop_f32(C.c_void_p(cache.buf.data_ptr()), cache.buf.numel(), 0 if cache.dtype == np.uint16 else 1,
                                    cache.H, cache.W, float(bl), float(wp), C.c_void_p(patches.ctypes.data), B, ps, int(bool(clip)),
                                    _lib.ptr(hr), _lib.ptr(lr), _lib.ptr(sigma), _lib.stream()), "yond_rawcrop_f32")
    return hr, lr, sigma


class RawCropSource:
    """A set of clean raw frames as the trainer's batch / eval source (SID_Raw_Dataset's device path).  wbs: one white balance
    [r, 1, b] per frame; ccms: one matrix (or None) per frame, passed through to the evaluation item."""

    def __init__(self, paths, args, device, wbs, ccms=None, frames=None):
        self.args = dict(args)
        self.cache = FrameCache(paths, device, frames)
        self.h, self.w = self.cache.H // 2, self.cache.W // 2
        self.wbs = [np.asarray(w, np.float64) for w in wbs]
        self.ccms = list(ccms) if ccms is not None else [None] * len(self.wbs)
        self.bl, self.wp = float(self.args['bl']), float(self.args['wp'])
        self.lock_wb = self.args.get('lock_wb', False)
        self.clip = bool(self.args.get('clip', False))
        self.ps, self.cpi = int(self.args.get('patch_size', 0)), int(self.args.get('crop_per_image', 8))
        self.croptype = self.args.get('croptype', 'random')
        if self.args.get('mode') == 'train':
            check_crops(self.h, self.w, self.ps, self.cpi, self.croptype)

    def __len__(self):
        return len(self.cache.paths)

    def batch(self, idx, gen, key, slot0):
        """One training batch: frames `idx` drawn from `gen`, crop_per_image patches each, patch j of the batch on noise stream
        (key, slot0 * crop_per_image + j).  Returns the trainer's batch dict with device lr / hr / sigma for
        len(idx) * crop_per_image patches."""
        a = self.args
        items = [sample_item(gen, self.h, self.w, self.ps, self.cpi, self.croptype, a['sigma_min'], a['sigma_max'], self.lock_wb,
                             self.wbs[int(i)]) for i in idx]
        n = len(items) * self.cpi
        p = plan(self.cache.offsets(idx), items, self.cache.H, self.cache.W, self.ps, key, int(slot0) * self.cpi + np.arange(n))
        hr, lr, sigma = launch(self.cache, p, self.ps, self.bl, self.wp, clip=self.clip)
        return {'lr': lr, 'hr': hr, 'sigma': sigma, 'pattern': [it['pattern'] for it in items],
                'vst_aug': [it['vst_aug'] for it in items], 'wb': [it['wb'] for it in items]}

    def item(self, idx, sigma):
        """Eval item `idx`: the whole frame as one patch [1][4][h'][w'] under eval_draws(idx), the fixed sigma, noise key idx:
        every pass gets the same item.  The export cuts square patches, so the frame is cut into its largest square tiles (side
        gcd(h', w'), tile t on noise slot t) and put together again."""
        d = dict(eval_draws(idx, self.wbs[idx], self.lock_wb), sigma=float(sigma))
        k = d['pattern']
        ho, wo = (self.w, self.h) if k & 1 else (self.h, self.w)
        g = math.gcd(ho, wo)
        ny, nx = ho // g, wo // g
        if ny * nx > 65536:
            raise ValueError(f"a {ho} x {wo} packed frame has no square tiling coarser than {g}: evaluate frames whose packed sides "
                             "share a larger factor")
        d['y0'] = [t // nx * g for t in range(ny * nx)]
        d['x0'] = [t % nx * g for t in range(ny * nx)]
        p = plan(self.cache.offsets([idx]), [d], self.cache.H, self.cache.W, g, idx, np.arange(ny * nx))
        hr, lr, s = launch(self.cache, p, g, self.bl, self.wp, clip=self.clip)
        whole = lambda t: t.view(ny, nx, 4, g, g).permute(2, 0, 3, 1, 4).reshape(1, 4, ho, wo)
        return {'lr': whole(lr), 'hr': whole(hr), 'sigma': s[:1], 'pattern': k, 'vst_aug': d['vst_aug'], 'wb': d['wb'],
                'ccm': self.ccms[idx]}


def check_crops(h, w, patch_size, crop_per_image, croptype):
    """What a training set must satisfy before its first batch: the patch fits, and a 'non-overlapped' grid has a cell for every
    crop (the reference would index past its list of origins)."""
    if patch_size < 1 or patch_size > min(h, w):
        raise ValueError(f"patch_size {patch_size} does not fit the packed frame {h} x {w} (both rotations are drawn)")
    cells = (h // patch_size) * (w // patch_size)
    if croptype == 'non-overlapped' and crop_per_image > cells:
        raise ValueError(f"croptype 'non-overlapped' with crop_per_image {crop_per_image}: a {h} x {w} packed frame has only "
                         f"{cells} cells of {patch_size} x {patch_size}")
