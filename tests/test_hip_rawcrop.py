"""GPU: yond_rawcrop_f32 (csrc/rawcrop.hip) -- bit equality with the float model (tests/rawcrop_model.py) on the reference's items
(tests/golden/rawcrop.npz) and on a seeded sweep of the smallest shapes that reach every path, batch / single-patch equality, the
noise stream's statistics and keying, the clip, the refused arguments -- and trainer_AWGN on a directory of raw frames."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import rawcrop_model as M
from yond_public_amd import _lib
from yond_public_amd import img2raw as I
from yond_public_amd import rawcrop as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
BL, WP = 512., 16383.


def _cache(frames):
    c = R.FrameCache([f"frame{i}" for i in range(len(frames))], DEV, frames=list(frames))
    c.offsets(np.arange(len(frames)))
    return c


def _frames(rng, n, H, W, dtype=np.uint16):
    """DN from below bl to above wp, with bl and wp themselves among them; float32 frames carry fractional DN."""
    out = []
    for _ in range(n):
        f = rng.integers(300, 16600, (H, W)).astype(np.float64)
        f.reshape(-1)[rng.choice(f.size, 4, replace=False)] = [BL, WP, 0, 65535]
        out.append(f.astype(np.uint16) if dtype == np.uint16 else (f + rng.random((H, W))).astype(np.float32))
    return out


def _item(pattern, vst_aug, y0, x0, rgb_gain=1., gain0=1., gain2=1., sigma=0.1):
    return dict(pattern=pattern, vst_aug=vst_aug, y0=list(y0), x0=list(x0), rgb_gain=np.float32(rgb_gain), gain0=gain0, gain2=gain2,
                sigma=sigma)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def test_hr_equals_the_model_on_the_reference_items(golden):
    g = golden("rawcrop")
    n = 0
    for c in M.golden_cases(g, "train"):
        rgb, g0, g2 = M.case_gains(c)
        H, W = c["bayer"].shape
        cache = _cache([c["bayer"]])
        p = R.plan([0], [_item(c["pattern"], c["vst_aug"], c["y0"], c["x0"], rgb, g0, g2, c["sigma"])], H, W, c["patch_size"], 3,
                   np.arange(len(c["y0"])))
        hr, lr, sig = R.launch(cache, p, c["patch_size"], BL, WP, clip=bool(c["clip"]))
        want = M.patches_hr(c["bayer"], BL, WP, c["pattern"], c["vst_aug"], c["y0"], c["x0"], c["patch_size"], rgb, g0, g2, c["clip"])
        assert np.array_equal(_bits(hr), want.view(np.uint32)), c["name"]
        assert np.array_equal(_bits(hr), c["hr"].view(np.uint32)), c["name"]        # the reference's own bits too
        assert np.array_equal(sig.cpu().numpy(), np.full(len(c["y0"]), np.float32(c["sigma"])))
        n += 1
    assert n == 48


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("shape", [(12, 20), (20, 12)])
def test_hr_equals_the_model_on_a_seeded_sweep(dtype, shape):
    """All four patterns x the four corners of the rotated frame x ps in {1, 3, 4, 5} x vst_aug x gains, as batches of 1, 3 and
    65 patches (65 = more than one chunk of the launch)."""
    rng = np.random.default_rng(17)
    H, W = shape
    frames = _frames(rng, 3, H, W, dtype)
    cache = _cache(frames)
    checked = 0
    for ps in (1, 3, 4, 5):
        items, offs, fidx = [], [], []
        for k in range(4):
            ho, wo = (W // 2, H // 2) if k & 1 else (H // 2, W // 2)
            for y0, x0 in ((0, 0), (0, wo - ps), (ho - ps, 0), (ho - ps, wo - ps)):
                for vst in (0, 1):
                    for gains in ((1., 1., 1.), (float(np.float32(rng.uniform(0.2, 1.6))), rng.uniform(0.6, 1.4), rng.uniform(0.6, 1.4))):
                        f = int(rng.integers(3))
                        items.append(_item(k, vst, [y0], [x0], *gains))
                        fidx.append(f)
        assert len(items) == 64
        items.append(_item(2, 1, [1], [0], 0.5, 1.25, 0.75))              # patch 65
        fidx.append(1)
        offs = cache.offsets(fidx)
        for B in (1, 3, 65):
            for clip in ((0, 1) if B == 65 else (0,)):
                p = R.plan(offs[:B], items[:B], H, W, ps, 9, np.arange(B))
                hr, _, _ = R.launch(cache, p, ps, BL, WP, clip=clip)
                got = _bits(hr)
                for b in range(B):
                    it = items[b]
                    want = M.patches_hr(frames[fidx[b]], BL, WP, it["pattern"], it["vst_aug"], it["y0"], it["x0"], ps, it["rgb_gain"],
                                        it["gain0"], it["gain2"], clip)
                    assert np.array_equal(got[b], want[0].view(np.uint32)), (ps, B, b, it)
                    checked += 1
    assert checked == 4 * (1 + 3 + 2 * 65)


def test_batch_equals_single_patch_launches():
    rng = np.random.default_rng(5)
    H, W, ps, cpi = 32, 48, 8, 8
    cache = _cache(_frames(rng, 8, H, W))
    gen, key = I.train_streams(2, 0)                  # epoch 2's stream: all four patterns, both coin outcomes, both vst_aug
    items = [R.sample_item(gen, H // 2, W // 2, ps, cpi, "random", 5, 50, wb=(2.0, 1.0, 1.6)) for _ in range(8)]
    assert len({it["pattern"] for it in items}) == 4 and len({it["gains"] is None for it in items}) == 2
    assert len({it["vst_aug"] for it in items}) == 2
    offs = cache.offsets(rng.permutation(8))
    p = R.plan(offs, items, H, W, ps, key, np.arange(64) + 100)
    assert len(p) == 64
    hr, lr, sig = R.launch(cache, p, ps, BL, WP, clip=True)
    for b in range(64):
        h1, l1, s1 = R.launch(cache, p[b:b + 1], ps, BL, WP, clip=True)
        assert torch.equal(h1[0], hr[b]) and torch.equal(l1[0], lr[b]) and torch.equal(s1[0], sig[b]), b
    # ... and whatever the buffers' alignment: a view 4 bytes into an allocation takes the narrow stores
    base_h, base_l = torch.zeros(hr.numel() + 1, device=DEV), torch.zeros(hr.numel() + 1, device=DEV)
    h2, l2, _ = R.launch(cache, p, ps, BL, WP, clip=True, hr=base_h[1:].view(hr.shape), lr=base_l[1:].view(hr.shape))
    assert torch.equal(h2, hr) and torch.equal(l2, lr) and base_h[0] == 0 and base_l[0] == 0


def _noise(cache, H, W, ps, key, slots, sigma=0.1, clip=False):
    items = [_item(s % 4, 0, [s % 3], [(2 * s) % 5], sigma=sigma) for s in range(len(slots))]
    p = R.plan(cache.offsets([0] * len(slots)), items, H, W, ps, key, slots)
    hr, lr, _ = R.launch(cache, p, ps, BL, WP, clip=clip)
    return hr, lr


def test_noise_statistics():
    """Five-sigma bounds of the sampling distributions of N = 8 * 4 * 24 * 24 independent standard normals (not measurements):
    the mean has standard deviation 1 / sqrt(N), the variance sqrt(2 / N), a correlation coefficient 1 / sqrt(N)."""
    rng = np.random.default_rng(7)
    H, W, ps = 64, 96, 24
    cache = _cache(_frames(rng, 1, H, W))
    sigma = 0.1
    hr, lr = _noise(cache, H, W, ps, 99, np.arange(8), sigma)
    z = ((lr - hr).double() / float(np.float32(sigma)))
    N = z.numel()
    assert N == 8 * 4 * 24 * 24
    m, v = z.mean().item(), z.var().item()
    a, b = z[..., :-1].flatten(), z[..., 1:].flatten()
    lag1 = torch.corrcoef(torch.stack([a, b]))[0, 1].item()
    slots = torch.corrcoef(torch.stack([z[:4].flatten(), z[4:].flatten()]))[0, 1].item()
    print(f"noise over {N} samples: mean {m:.3e}, var {v:.5f}, lag-1 corr {lag1:.3e}, slot corr {slots:.3e}; bound {5 / math.sqrt(N):.3e}")
    assert abs(m) <= 5 / math.sqrt(N)
    assert abs(v - 1) <= 5 * math.sqrt(2 / N)
    assert abs(lag1) <= 5 / math.sqrt(N)
    assert abs(slots) <= 5 / math.sqrt(N)                       # slots 0..3 against slots 4..7, element by element
    two = torch.corrcoef(torch.stack([z[0].flatten(), z[1].flatten()]))[0, 1].item()
    assert abs(two) <= 5 / math.sqrt(N), two                    # two neighbouring slots, held to the same bound
    for s in range(1, 8):                                       # slot 0 against every other: five sigma of N / 8 samples each
        r = torch.corrcoef(torch.stack([z[0].flatten(), z[s].flatten()]))[0, 1].item()
        assert abs(r) <= 5 / math.sqrt(N / 8), (s, r)


def test_noise_keying():
    rng = np.random.default_rng(6)
    H, W, ps = 64, 96, 24
    cache = _cache(_frames(rng, 1, H, W))
    h0, l0 = _noise(cache, H, W, ps, 7, [0, 1])
    h1, l1 = _noise(cache, H, W, ps, 7, [0, 1])
    assert torch.equal(l0, l1) and torch.equal(h0, h1)
    for key, slots in ((8, [0, 1]), (7, [2, 3])):
        h2, l2 = _noise(cache, H, W, ps, key, slots)
        assert torch.equal(h2, h0)                                        # hr is untouched by the noise stream
        assert not torch.equal(l2[0], l0[0]) and not torch.equal(l2[1], l0[1])
    h3, l3 = _noise(cache, H, W, ps, 7, [1, 0])                          # the stream belongs to (key, slot), not to the position
    assert not torch.equal(l3[0] - h3[0], l0[0] - h0[0])


def test_clip():
    rng = np.random.default_rng(8)
    H, W, ps = 64, 96, 24
    cache = _cache(_frames(rng, 1, H, W))
    items = [_item(k, k & 1, [k], [k], 1.5, 1.4, 1.3, sigma=0.5) for k in range(4)]        # gains push hr past 1, sigma lr past both ends
    p = R.plan(cache.offsets([0] * 4), items, H, W, ps, 1, np.arange(4))
    hr, lr, _ = R.launch(cache, p, ps, BL, WP, clip=False)
    hc, lc, _ = R.launch(cache, p, ps, BL, WP, clip=True)
    assert hr.max().item() > 1 and lr.max().item() > 1 and lr.min().item() < 0
    assert torch.equal(hc, hr.clamp(0, 1)) and torch.equal(lc, lr.clamp(0, 1))
    assert 0 <= lc.min().item() and lc.max().item() <= 1


def test_bad_arguments_return_einval_and_write_nothing():
    rng = np.random.default_rng(9)
    H, W, ps = 12, 20, 4
    cache = _cache(_frames(rng, 2, H, W))
    lib = _lib.load()
    good = R.plan(cache.offsets([1, 0]), [_item(1, 0, [6], [2]), _item(0, 1, [2], [6])], H, W, ps, 1, [0, 1])
    hr = torch.full((2, 4, ps, ps), -7.0, device=DEV)
    lr, sig = torch.full_like(hr, -7.0), torch.full((2,), -7.0, device=DEV)

    def call(frames=cache.buf.data_ptr(), flen=cache.buf.numel(), dtype=0, H=H, W=W, patches=good, B=2, ps=ps, hr=hr, lr=lr, sig=sig):
        pp = None if patches is None else C.c_void_p(np.ascontiguousarray(patches).ctypes.data)
        return lib.yond_rawcrop_f32(None if frames is None else C.c_void_p(frames), flen, dtype, H, W, BL, WP, pp, B, ps, 1, _lib.ptr(hr),
                                    _lib.ptr(lr), _lib.ptr(sig), _lib.stream())

    def patched(i, **kw):
        p = good.copy()
        for k, v in kw.items():
            p[k][i] = v
        return p
    bad = [dict(frames=None), dict(patches=None), dict(hr=None), dict(lr=None), dict(sig=None),
           dict(H=11), dict(W=19), dict(ps=0), dict(ps=-1), dict(B=0), dict(dtype=2),
           dict(patches=patched(0, y0=7)), dict(patches=patched(0, x0=3)), dict(patches=patched(1, y0=3)), dict(patches=patched(1, x0=7)),
           dict(patches=patched(1, y0=-1)), dict(patches=patched(0, x0=-1)), dict(patches=patched(1, pattern=1)),   # 0 -> 1 swaps the bounds
           dict(patches=patched(0, pattern=4)), dict(patches=patched(1, vst_aug=2)),
           dict(patches=patched(0, frame=H * W + 1)), dict(patches=patched(1, frame=-1)), dict(flen=2 * H * W - 1)]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (hr == -7).all() and (lr == -7).all() and (sig == -7).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert (hr != -7).all() and (lr != -7).all() and np.array_equal(sig.cpu().numpy(), good["sigma"])
    with pytest.raises(Exception, match="ROCm device"):
        R.FrameCache(["x"], "cpu", frames=[np.zeros((2, 2), np.uint16)])


# -- trainer_AWGN on raw frames -----------------------------------------------------------------------------------------------
def _sid_runfile(tmp_path, root):
    import yaml
    cfg = yaml.load(open(os.path.join(ROOT, "runfiles", "Gaussian", "GRU_5to50_norm_sid.yml")).read(), Loader=yaml.FullLoader)
    cfg["arch"]["nf"] = 8
    for sec in ("dst", "dst_train", "dst_eval", "dst_test"):
        cfg[sec].update(H=64, W=96, patch_size=32, crop_per_image=4, root_dir=str(root))
    cfg["hyper"].update(batch_size=2, last_epoch=0, stop_epoch=2, step_size=1, T=1, coldstart=True, save_freq=1, plot_freq=1,
                        learning_rate=5e-3)
    rf = tmp_path / "sid.yml"
    rf.write_text(yaml.dump(cfg))
    return str(rf), cfg


def _check_run(tmp_path, argv, cfg):
    from yond_public_amd import trainer_AWGN as TA
    out = TA.main(argv)
    hist = out["history"]
    assert [h[0] for h in hist] == [1, 2] and all(len(h[2]) == 3 for h in hist)          # 6 frames / batch size 2
    losses = np.array([h[2] for h in hist]).reshape(-1)
    assert np.isfinite(losses).all() and len(set(losses.tolist())) == len(losses)
    name = cfg["model_name"]
    for f in (f"checkpoints/Gaussian/{name}_last_model.pth", f"checkpoints/Gaussian/{name}_best_model.pth",
              f"saved_model/Gaussian/{name}_e0002.pth"):
        assert os.path.exists(tmp_path / f), f
    assert all(np.isfinite(out[f"psnr_sig{s}"]) and np.isfinite(out[f"ssim_sig{s}"]) for s in (10, 25, 50))
    tr = TA.AWGN_Trainer(argv[:2] + ["-m", "train"] + argv[4:])
    assert tr.step_batch == 8 and isinstance(tr.src_train, R.RawCropSource) and isinstance(tr.src_eval, R.RawCropSource)
    gen, key = I.train_streams(1, 0)
    data = tr.src_train.batch(np.array([0, 5]), gen, key, 0)
    assert tuple(data["lr"].shape) == tuple(data["hr"].shape) == (8, 4, 32, 32) and tuple(data["sigma"].shape) == (8,)
    item = tr.src_eval.item(1, 25 / 255.)
    assert tuple(item["hr"].shape) == (1, 4, 48, 32) and item["pattern"] == 1              # the whole rotated frame
    tr.dst_eval.sigma = 25 / 255.
    m1 = dict(tr.eval(-1))
    m2 = dict(tr.eval(-1))
    assert m1 == m2 and len(m1) >= 6                                                      # the same items every pass
    return tr


def test_trainer_awgn_on_raw_frames(tmp_path, monkeypatch):
    """`trainer_AWGN -f runfile -m train` on a directory of six 64 x 96 uint16 frames: batches cut on the device, two epochs,
    checkpoints, evaluation, and an evaluation pass that repeats."""
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(11)
    rng = np.random.default_rng(12)
    y, x = np.mgrid[0:64, 0:96]
    for d in ("train", "eval", "test"):
        (tmp_path / "data" / d).mkdir(parents=True)
        for i in range(6):
            f = 0.5 + 0.45 * np.sin(rng.uniform(0.02, 0.1) * y + rng.uniform(0.02, 0.1) * x + rng.uniform(0, 6))
            np.save(tmp_path / "data" / d / f"frame{i}.npy", np.round(BL + (WP - BL) * f).astype(np.uint16))
    rf, cfg = _sid_runfile(tmp_path, tmp_path / "data")
    tr = _check_run(tmp_path, ["-f", rf, "-m", "train"], cfg)
    whole = tr.src_eval.item(0, 25 / 255.)["hr"][0].cpu().numpy()
    frame = np.load(tmp_path / "data" / "eval" / "frame0.npy")
    d = R.eval_draws(0)
    want = M.frame_hr(frame, BL, WP, 0, 0)[None] * d["rgb_gain"]
    want[:, 0] = (want[:, 0].astype(np.float64) * d["gain0"]).astype(np.float32)
    want[:, 2] = (want[:, 2].astype(np.float64) * d["gain2"]).astype(np.float32)
    assert np.array_equal(whole, want[0].clip(0, 1))                                      # the tiles went back where they belong


def test_trainer_awgn_on_synthetic_frames(tmp_path, monkeypatch):
    """The same run under --synthetic 6 with no directory."""
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(11)
    rf, cfg = _sid_runfile(tmp_path, tmp_path / "nothing")
    _check_run(tmp_path, ["-f", rf, "-m", "train", "--synthetic", "6"], cfg)
