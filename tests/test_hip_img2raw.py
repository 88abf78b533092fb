"""GPU: yond_img2raw_f32 (csrc/img2raw.hip) -- the reference's sRGB -> raw items (tests/golden/img2raw.npz), batch / single-crop
equality, the noise stream's keying and statistics -- and trainer_AWGN on a directory of sRGB crops."""
import os

import numpy as np
import pytest
import torch

from yond_public_amd import img2raw as I

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _cache(tmp_path, crops, name="c"):
    d = tmp_path / name
    d.mkdir()
    for i, c in enumerate(crops):
        np.save(d / f"{i:03d}.npy", c)
    return I.CropCache(sorted(str(p) for p in d.glob("*.npy")), DEV)


def _crops(rng, n, H, W, dtype=np.uint8, texture=0.05, fmax=0.2):
    top = np.iinfo(dtype).max
    y, x = np.mgrid[0:H, 0:W]
    out = []
    for _ in range(n):
        f = rng.uniform(0.02, fmax, (3, 2))
        base = 0.5 + 0.5 * np.sin(f[:, :1, None] * y + f[:, 1:, None] * x + rng.uniform(0, 6, (3, 1, 1)))
        img = np.clip(base.transpose(1, 2, 0) + rng.normal(0, texture, (H, W, 3)), 0, 1)
        out.append(np.round(img * top).astype(dtype))
    return out


def test_hr_matches_the_reference(golden, tmp_path):
    g = golden("img2raw")
    worst = {}
    cases = [(k, "eval") for k in g["eval_cases"]] + [(k, "explicit") for k in g["explicit_cases"]]
    for n, (key, kind) in enumerate(cases):
        crop = g[key + "_crop"]
        cache = _cache(tmp_path, [crop], f"c{n}")
        table = I.curve(crop.dtype, float(g[key + "_divisor"]), DEV)
        if kind == "eval":
            lw = g[key + "_lock_wb"]
            meta = I.eval_meta(int(g[key + "_idx"]), False if lw.size == 0 else lw.reshape(3, 1).tolist())
        else:
            rg, red, blue = (torch.tensor([v]) for v in g[key + "_gains"])
            meta = {"rgb2cam": torch.from_numpy(g[key + "_rgb2cam"]), "rgb_gain": rg, "red": red, "blue": blue}
        k = int(g[key + "_pattern"])
        p = I.plan(cache.offsets([0]), [meta], [k], [25 / 255.], 1, [0])
        hr, lr, sig = I.launch(cache, table, p, pattern=k, clip=True)
        torch.cuda.synchronize()
        ref = g[key + "_hr"]
        assert tuple(hr.shape[1:]) == ref.shape, key
        worst[key] = float(np.abs(hr[0].cpu().numpy() - ref).max())
        assert sig.item() == np.float32(25 / 255.)
        assert 0 <= lr.min().item() and lr.max().item() <= 1
    print("max |hr - reference| per case:", {k: f"{v:.2e}" for k, v in worst.items()})
    print(f"max over all cases: {max(worst.values()):.3e}")
    assert max(worst.values()) <= 2e-6, worst


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_batch_equals_single_crop_launches(tmp_path, dtype):
    rng = np.random.default_rng(5)
    B = 64
    cache = _cache(tmp_path, _crops(rng, B, 32, 32, dtype))
    table = I.curve(dtype, 255. if dtype == np.uint8 else 65535., DEV)
    gen, key = I.train_streams(1, 0)
    draws = [I.sample_item(gen, 5, 50) for _ in range(B)]
    metas, pats, sigs = zip(*draws)
    assert len(set(pats)) == 4
    idx = rng.permutation(B)
    p = I.plan(cache.offsets(idx), metas, pats, sigs, key, np.arange(B) + 100)
    hr, lr, sig = I.launch(cache, table, p, pattern=-1, clip=True)
    for b in range(B):
        h1, l1, s1 = I.launch(cache, table, p[b:b + 1], pattern=int(pats[b]), clip=True)
        assert torch.equal(h1[0], hr[b]) and torch.equal(l1[0], lr[b]) and torch.equal(s1[0], sig[b]), b


def test_noise_keying(tmp_path):
    rng = np.random.default_rng(6)
    cache = _cache(tmp_path, _crops(rng, 1, 256, 256))
    table = I.curve(np.uint8, 255., DEV)
    meta = I.eval_meta(3)

    def noise(key, slot):
        p = I.plan(cache.offsets([0]), [meta], [2], [0.1], key, [slot])
        hr, lr, _ = I.launch(cache, table, p, pattern=2, clip=False)
        return lr - hr
    a = noise(7, 0)
    assert torch.equal(a, noise(7, 0))
    for other in (noise(8, 0), noise(7, 1)):
        assert not torch.equal(a, other)
        assert abs(torch.corrcoef(torch.stack([a.flatten(), other.flatten()]))[0, 1].item()) < 0.02     # 65536 samples: 5 sigma


def test_noise_statistics(tmp_path):
    rng = np.random.default_rng(7)
    B = 64
    cache = _cache(tmp_path, _crops(rng, B, 256, 256))
    table = I.curve(np.uint8, 255., DEV)
    metas = [I.eval_meta(i) for i in range(B)]
    p = I.plan(cache.offsets(np.arange(B)), metas, [i % 4 for i in range(B)], [1.0] * B, 99, np.arange(B))
    hr, lr, _ = I.launch(cache, table, p, pattern=-1, clip=False)
    z = ((lr - hr) / 1.0).double().flatten()                          # [patch][channel][y][x]: lag 1 crosses all three
    n = z.numel()
    assert n >= 4 * 2 ** 20
    m, v = z.mean().item(), z.var().item()
    c = z - m
    kurt = (c ** 4).mean().item() / v ** 2
    lag1 = ((c[1:] * c[:-1]).mean() / v).item()
    tail = (z.abs() > 3).double().mean().item()
    print(f"noise over {n} samples: mean {m:.2e}, var {v:.5f}, kurtosis {kurt:.4f}, lag-1 corr {lag1:.2e}, 3-sigma tail {tail:.5f}")
    assert abs(m) < 3e-3 and abs(v - 1) < 5e-3 and abs(kurt - 3) < 0.03 and abs(lag1) < 3e-3
    assert abs(tail - 0.0027) < 3e-4
    hc, lc, _ = I.launch(cache, table, p, pattern=-1, clip=True)
    assert hc.min().item() >= 0 and hc.max().item() <= 1 and lc.min().item() >= 0 and lc.max().item() <= 1
    assert torch.equal(hc, hr)                                       # hr is already in [0, 1]


def test_cpu_tensors_raise(tmp_path):
    with pytest.raises(Exception, match="ROCm device"):
        I.CropCache([], "cpu")


# -- trainer_AWGN on sRGB crops -----------------------------------------------------------------------------------------------
def _srgb_runfile(tmp_path, src, **hyper_over):
    import yaml
    cfg = yaml.load(open(os.path.join(ROOT, "runfiles", "Gaussian", src)).read(), Loader=yaml.FullLoader)
    cfg["arch"]["nf"] = 8
    for sec in ("dst", "dst_train", "dst_eval", "dst_test"):
        cfg[sec].update(H=64, W=64, patch_size=64, root_dir=str(tmp_path / "data"))
    cfg["hyper"].update(batch_size=4, last_epoch=0, stop_epoch=40, step_size=1, T=1, coldstart=True, save_freq=10, plot_freq=10,
                        learning_rate=5e-3)
    cfg["hyper"].update(hyper_over)
    rf = tmp_path / ("srgb_" + src)
    rf.write_text(yaml.dump(cfg))
    return str(rf), cfg


def _srgb_dirs(tmp_path, dirs, n=16):
    rng = np.random.default_rng(11)
    crops = _crops(rng, n, 64, 64, texture=0.0, fmax=0.1)           # smooth scenes: what is left after denoising is the noise
    for d in dirs:
        (tmp_path / "data" / d).mkdir(parents=True, exist_ok=True)
        for i, c in enumerate(crops):
            np.save(tmp_path / "data" / d / f"crop{i:02d}.npy", c)


def test_trainer_awgn_on_srgb_crops(tmp_path, monkeypatch):
    """`trainer_AWGN -f runfile -m train` on a directory of sRGB crops (no --synthetic): the batches are synthesised on the device,
    the network learns to denoise, and a fresh evaluation pass reproduces the logged PSNR."""
    from yond_public_amd import archs as A
    from yond_public_amd import trainer_AWGN as TA
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(11)
    _srgb_dirs(tmp_path, ("train_mix", "eval", "test"))
    rf, cfg = _srgb_runfile(tmp_path, "GRU_5to50_norm_mix.yml", stop_epoch=80)
    out = TA.main(['-f', rf, '-m', 'train'])
    hist = out['history']
    assert [h[0] for h in hist] == list(range(1, 81)) and all(len(h[2]) == 4 for h in hist)
    assert all(np.isfinite(h[2]).all() for h in hist)
    assert out['psnr_sig10'] > out['psnr_sig25'] > out['psnr_sig50'] > 10
    name = cfg['model_name']
    net = A.GuidedResUnet(dict(cfg['arch']))
    net.load_state_dict(torch.load(f"checkpoints/Gaussian/{name}_best_model.pth", map_location='cpu'))
    net = net.to(DEV).eval()
    tr = TA.AWGN_Trainer(['-f', rf, '-m', 'eval'])
    assert tr.src_eval is not None
    tr.net = net
    tr.dst_eval.sigma = 25 / 255.
    tr.eval(-1)
    assert abs(tr.eval_psnr.avg - out['psnr_sig25']) < 1e-6            # fresh pass, same items, same PSNR
    ps_in = []
    for k in range(len(tr.dst_eval)):
        d = tr.src_eval.item(k, 25 / 255.)
        ps_in.append(TA.quality_assess(d['lr'] * 255, d['hr'] * 255)['PSNR'])
    print(f"sRGB crops, sigma 25: input {np.mean(ps_in):.2f} dB -> denoised {out['psnr_sig25']:.2f} dB after 320 steps")
    assert out['psnr_sig25'] > np.mean(ps_in) + 1.5


def test_trainer_refuses_mixed_and_non_square(tmp_path, monkeypatch):
    from yond_public_amd import trainer_AWGN as TA
    monkeypatch.chdir(tmp_path)
    _srgb_dirs(tmp_path, ("train_mix", "eval"), n=4)
    np.save(tmp_path / "data" / "train_mix" / "packed.npy", np.zeros((4, 32, 32), np.float32))
    rf, _ = _srgb_runfile(tmp_path, "GRU_5to50_norm_mix.yml")
    with pytest.raises(ValueError, match="sRGB crops.*packed raw"):
        TA.AWGN_Trainer(['-f', rf, '-m', 'train'])
    os.remove(tmp_path / "data" / "train_mix" / "packed.npy")
    for f in (tmp_path / "data" / "train_mix").glob("*.npy"):
        np.save(f, np.zeros((64, 32, 3), np.uint8))
    with pytest.raises(ValueError, match="non-square"):
        TA.AWGN_Trainer(['-f', rf, '-m', 'train'])


def test_trainer_awgn_unet_srgb_under_torchrun(tmp_path):
    """The UNet runfile (DIV2K_Img2Raw_Dataset, crops under the reference's <root>/npy/<mode>) as a one-rank torchrun job."""
    import subprocess
    import sys
    _srgb_dirs(tmp_path, ("npy/train", "npy/eval", "npy/test"), n=8)
    rf, cfg = _srgb_runfile(tmp_path, "Unet_5to50_norm.yml", stop_epoch=2, save_freq=1, plot_freq=1)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", "29571", os.path.join(ROOT, "trainer_AWGN.py"), "-f", rf, "-m", "train"]
    out = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    assert "Epoch 2:" in out.stdout and "AWGN Datasets: sigma=50" in out.stdout
    assert os.path.exists(tmp_path / "checkpoints" / "Gaussian" / f"{cfg['model_name']}_last_model.pth")
