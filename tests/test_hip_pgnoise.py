"""GPU: yond_pg_noise_f32 (csrc/pgnoise.hip) -- the Poisson sampler's distribution over every regime and threshold, the counter-based
contract (an element's value depends on its item, its index and its clean value only), the edge rules of include/yond_hip.h, the
Gaussian term, the keying -- then DIV2K_PG_Dataset in trainer_AWGN and --synth-noise in the full-frame driver.
A fixed key makes every statistical check deterministic.  Bounds: 5 standard errors of the statistic under the exact law, chi-square
at a 1e-6 tail (tests/pgnoise_stats.py)."""
import os

import numpy as np
import pytest
import torch

import pgnoise_stats as PS
from yond_public_amd import pgnoise as PG

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
BETA1 = 2.0 ** -6
KEY = 20261018


def _ladder():
    return PS.ladder(PG.SWITCH_LAMBDAS)


def _const(lam, n, key=KEY, slot=0, sigma=0.0):
    """One launch of n elements of constant x = lam * BETA1 (exact: BETA1 is a power of two)."""
    clean = torch.full((n,), float(np.float32(lam) * np.float32(BETA1)), dtype=torch.float32, device=DEV)
    return PG.add_pg_noise(clean, BETA1, sigma, 1.0, key, [slot])


@pytest.fixture(scope="module")
def const_launches():
    """The constant-lambda launches of 2^18 elements, one per ladder value, all with (KEY, slot 0): shared, never modified."""
    out = [_const(lam, 2 ** 18) for lam in _ladder()]
    torch.cuda.synchronize()
    return out


def test_ladder_distribution(const_launches):
    bad = []
    for lam, noisy in zip(_ladder(), const_launches):
        k = noisy.double().cpu().numpy() / BETA1
        row, fails = PS.check_counts(k, lam)
        print(row + ("   FAIL: " + "; ".join(fails) if fails else ""))
        bad += [f"lambda {lam}: {f}" for f in fails]
    assert not bad, bad


def test_value_depends_only_on_element(const_launches):
    lams = np.array(_ladder(), np.float32)
    L, n = len(lams), 2 ** 16
    x = torch.from_numpy(np.tile(lams * np.float32(BETA1), n // L + 1)[:n].copy()).to(DEV)
    mixed = PG.add_pg_noise(x, BETA1, 0.0, 1.0, KEY, [0])
    ref = torch.empty_like(mixed)                                    # element i from the constant launch of its lambda
    for j, c in enumerate(const_launches):
        ref[j::L] = c[:n][j::L]
    assert torch.equal(mixed, ref)
    regimes = np.digitize(lams, PG.SWITCH_LAMBDAS)
    assert set(regimes) == {0, 1, 2} and L < 64                      # every regime inside every wavefront

    # item 3 of a batch of 5 (the others: other slots, other data)
    batch = torch.rand(5, n, device=DEV)
    batch[3] = x
    slots = [7, 8, 9, 0, 11]
    out = PG.add_pg_noise(batch, BETA1, 0.0, 1.0, KEY, slots)
    assert torch.equal(out[3], mixed)
    assert not torch.equal(out[2], mixed)
    # shorter items: the first n' elements are the same whatever n_per_item is
    for m in (1000, 1, 3, 4, 5, 1023, 1025):
        assert torch.equal(PG.add_pg_noise(x[:m].clone(), BETA1, 0.0, 1.0, KEY, [0]), mixed[:m]), m
    # views starting one float into a buffer: clean only, noisy only, both
    buf_in = torch.zeros(n + 8, device=DEV)
    buf_in[1:n + 1] = x
    buf_out = torch.full((n + 8,), -7.0, device=DEV)
    for cin, cout in ((buf_in[1:n + 1], None), (x, buf_out[1:n + 1]), (buf_in[1:n + 1], buf_out[1:n + 1]),
                      (buf_in[1:1026], buf_out[3:1028])):
        got = PG.add_pg_noise(cin, BETA1, 0.0, 1.0, KEY, [0], out=cout)
        assert torch.equal(got, mixed[:cin.numel()])
        if cout is not None:                                         # nothing written outside the view
            lo = (cout.data_ptr() - buf_out.data_ptr()) // 4
            assert (buf_out[:lo] == -7.0).all() and (buf_out[lo + cout.numel():] == -7.0).all()
            buf_out.fill_(-7.0)
    # in place, aligned and not
    y = x.clone()
    assert PG.add_pg_noise(y, BETA1, 0.0, 1.0, KEY, [0], out=y) is y and torch.equal(y, mixed)
    v = buf_in[1:n + 1]
    PG.add_pg_noise(v, BETA1, 0.0, 1.0, KEY, [0], out=v)
    assert torch.equal(v, mixed) and buf_in[0] == 0 and (buf_in[n + 1:] == 0).all()


def _z_stats(z):
    z = z.double().flatten()
    m, v = z.mean().item(), z.var().item()
    c = z - m
    return m, v, (c ** 4).mean().item() / v ** 2, ((c[1:] * c[:-1]).mean() / v).item(), (z.abs() > 3).double().mean().item()


def _assert_standard_normal(z, what):
    """The bounds of tests/test_hip_img2raw.py test_noise_statistics (4 * 2^20 samples)."""
    assert z.numel() >= 4 * 2 ** 20
    m, v, kurt, lag1, tail = _z_stats(z)
    print(f"{what} over {z.numel()} samples: mean {m:.2e}, var {v:.5f}, kurtosis {kurt:.4f}, lag-1 corr {lag1:.2e}, 3-sigma tail {tail:.5f}")
    assert abs(m) < 3e-3 and abs(v - 1) < 5e-3 and abs(kurt - 3) < 0.03 and abs(lag1) < 3e-3
    assert abs(tail - 0.0027) < 3e-4


def test_edges():
    n = 2 ** 16
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.rand(n, device=DEV, generator=g)
    # sigma_n = 0: integer counts
    k = PG.add_pg_noise(x, BETA1, 0.0, 1.0, KEY, [1]).double() / BETA1
    assert torch.equal(k, k.round()) and k.min() >= 0 and k.std() > 1
    # x < 0: read noise only, whatever beta1 says; the noise is the one a non-negative x gets at the same index
    s = 0.125
    neg = PG.add_pg_noise(torch.full((n,), -0.25, device=DEV), BETA1, s, 1.0, KEY, [1])
    zero = PG.add_pg_noise(torch.zeros(n, device=DEV), BETA1, s, 1.0, KEY, [1])
    assert torch.equal(neg, zero - 0.25)                            # s * z exact in both, -0.25 + s z: one rounding each
    m, v, kurt, lag1, tail = _z_stats((neg + 0.25) / s)
    assert abs(m) < 5 / np.sqrt(n) and abs(v - 1) < 5 * np.sqrt(2 / n) and abs(kurt - 3) < 5 * np.sqrt(24 / n)
    # NaN / +-inf exactly where they stand
    bad = {5: float("nan"), 64: float("inf"), 1001: float("-inf"), n - 1: float("nan")}
    xb = x.clone()
    for i, val in bad.items():
        xb[i] = val
    for b1, sig in ((BETA1, 0.01), (0.0, 0.01), (BETA1, 0.0)):
        yb = PG.add_pg_noise(xb, b1, sig, 1.0, KEY, [1])
        nan = torch.isnan(yb).nonzero().flatten().tolist()
        assert nan == sorted(bad) and torch.isfinite(yb).sum().item() == n - len(bad), (b1, sig, nan)
    # finite everywhere: huge x, denormal beta1 (lambda overflows), huge lambda
    ext = torch.tensor([0.0, 1e-30, 1.0, 3e38, 1e30, 65504.0, -3e38], device=DEV)
    for b1 in (BETA1, 1e-42, 1e-30, 1e30):
        ye = PG.add_pg_noise(ext, b1, 0.0, 1.0, KEY, [1])
        assert torch.isfinite(ye).all(), (b1, ye)
    # clip = 1 is clamp of clip = 0
    wide = (x * 3 - 1)
    free = PG.add_pg_noise(wide, 4 * BETA1, 0.2, 1.0, KEY, [2])
    clipped = PG.add_pg_noise(wide, 4 * BETA1, 0.2, 1.0, KEY, [2], clip=True)
    assert free.min() < 0 and free.max() > 1
    assert torch.equal(clipped, free.clamp(0, 1))
    # exposure: a power of two scales everything exactly
    e = 2.0 ** -7
    lo = PG.add_pg_noise(x, BETA1, 0.05, 1.0, KEY, [3], exposure=e)
    assert torch.equal(lo, PG.add_pg_noise(x * e, BETA1, 0.05, 1.0, KEY, [3]) / e)
    # exposure 1 / 100: the same counts as the exposure-1 launch on x * e (the product the kernel forms), scaled back within 1 ulp
    e = float(np.float32(0.01))
    lo = PG.add_pg_noise(x, BETA1 / 64, 0.0, 1.0, KEY, [3], exposure=e).double()
    full = PG.add_pg_noise(x * e, BETA1 / 64, 0.0, 1.0, KEY, [3]).double() / e
    ulp = torch.from_numpy(np.spacing(full.abs().float().cpu().numpy())).to(DEV).double()
    assert ((lo - full).abs() <= ulp).all()
    assert (lo - x.double()).std() > 0.08                           # 100 x fewer photons: visibly noisier than ...
    assert (PG.add_pg_noise(x, BETA1 / 64, 0.0, 1.0, KEY, [3]).double() - x.double()).std() < 0.02


def test_gaussian_and_total_variance():
    n = 2 ** 22
    g = torch.Generator(device=DEV).manual_seed(2)
    x = torch.rand(n, device=DEV, generator=g)
    s = 0.375
    for b1 in (0.0, -1.0):
        r = PG.add_pg_noise(x, b1, s, 1.0, KEY, [4]) - x
        _assert_standard_normal(r / s, f"beta1 {b1}: residual / sigma_n")
        frac = (r.double() / BETA1)
        assert ((frac - frac.round()).abs() < 1e-3).double().mean().item() < 0.01         # no lattice
    # shot + read noise of equal variance at lambda 50: Var(noisy / beta1) = 2 lambda unless the two draws are correlated
    lam = 50.0
    t = (_const(lam, n, slot=5, sigma=float(np.sqrt(lam) * BETA1)).double() / BETA1)
    var, se = t.var().item(), np.sqrt((lam + 8 * lam * lam) / n)
    print(f"lambda 50 + equal read noise: mean {t.mean().item():.4f}, var {var:.4f} vs {2 * lam} ({abs(var - 2 * lam) / se:.2f} se)")
    assert abs(var - 2 * lam) <= 5 * se
    assert abs(t.mean().item() - lam) <= 5 * np.sqrt(2 * lam / n)


def test_keying():
    n = 2 ** 18
    lim = 5 / np.sqrt(n)
    for lam in (3.0, 1e3):
        a = _const(lam, n, key=7, slot=0, sigma=BETA1)
        assert torch.equal(a, _const(lam, n, key=7, slot=0, sigma=BETA1))
        for other in (_const(lam, n, key=8, slot=0, sigma=BETA1), _const(lam, n, key=7, slot=1, sigma=BETA1)):
            assert not torch.equal(a, other)
            c = torch.corrcoef(torch.stack([a.double() - a.double().mean(), other.double() - other.double().mean()]))[0, 1].item()
            assert abs(c) < lim, (lam, c)
        k = _const(lam, n, key=7, slot=0).double() / BETA1 - lam
        lag1 = ((k[1:] * k[:-1]).mean() / (k * k).mean()).item()
        print(f"lambda {lam}: lag-1 autocorrelation of the counts {lag1:.2e} (< {lim:.2e})")
        assert abs(lag1) < lim


def test_cpu_tensors_raise():
    with pytest.raises(Exception, match="ROCm device"):
        PG.add_pg_noise(torch.zeros(16), 1.0, 1.0, 1.0, 0, [0])


# -- trainer_AWGN on DIV2K_PG_Dataset ------------------------------------------------------------------------------------------
def _pg_runfile(tmp_path, name="pg.yml", arch=None):
    import yaml
    load = lambda f: yaml.load(open(os.path.join(ROOT, "runfiles", "Gaussian", f)).read(), Loader=yaml.FullLoader)
    cfg = load("Unet_PG_norm_noclip.yml")
    if arch is not None:
        cfg["arch"] = load(arch)["arch"]
    cfg["arch"]["nf"] = 8
    for sec in ("dst", "dst_train", "dst_eval", "dst_test"):
        cfg[sec].update(H=64, W=64, patch_size=64, root_dir=str(tmp_path / "data"))
    cfg["hyper"].update(batch_size=8, last_epoch=0, stop_epoch=2, step_size=1, T=1, coldstart=True, save_freq=1, plot_freq=1,
                        learning_rate=1e-3)
    rf = tmp_path / name
    rf.write_text(yaml.dump(cfg))
    return str(rf), cfg


def _srgb_dirs(tmp_path, dirs, n=16, H=64, W=64):
    rng = np.random.default_rng(11)
    y, x = np.mgrid[0:H, 0:W]
    for i in range(n):
        f = rng.uniform(0.02, 0.1, (3, 2))
        img = 0.5 + 0.5 * np.sin(f[:, :1, None] * y + f[:, 1:, None] * x + rng.uniform(0, 6, (3, 1, 1)))
        crop = np.round(img.transpose(1, 2, 0) * 255).astype(np.uint8)
        for d in dirs:
            (tmp_path / "data" / d).mkdir(parents=True, exist_ok=True)
            np.save(tmp_path / "data" / d / f"crop{i:02d}.npy", crop)


def test_trainer_pg_dataset(tmp_path, monkeypatch):
    """`trainer_AWGN -f Unet_PG_norm_noclip.yml` (cut down) on 16 sRGB crops: the dataset resolves by name and trains; a batch's noise
    has the variance beta1 hr + beta2 of its item's own (K, sigma); evaluation items repeat bit for bit; a guided net is refused."""
    from yond_public_amd import img2raw as I
    from yond_public_amd import trainer_AWGN as TA
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(3)
    _srgb_dirs(tmp_path, ("train", "eval", "test"))
    rf, cfg = _pg_runfile(tmp_path)
    out = TA.main(['-f', rf, '-m', 'train'])
    hist = out['history']
    assert [h[0] for h in hist] == [1, 2] and all(len(h[2]) == 2 for h in hist)
    assert all(np.isfinite(h[2]).all() for h in hist)
    assert np.isfinite(out['psnr_pg']) and len(out['metrics_pg']) == 16

    tr = TA.AWGN_Trainer(['-f', rf, '-m', 'train'])
    assert type(tr.dst_train) is TA.DIV2K_PG_Dataset and type(tr.src_train).__name__ == 'PGSource'
    assert (tr.dst_eval.p['K'], tr.dst_eval.p['sigma']) == (2.0, 8.0)                     # the runfile's dst_eval.K / sigma_dn
    gen, key = I.train_streams(1, 0)
    idx = np.array([0, 1, 2, 3, 0, 1, 2, 3])                                              # every crop twice
    data = tr.src_train.batch(idx, gen, key, 0)
    hr, lr = data['hr'].double(), data['lr'].double()
    assert hr.shape == lr.shape == (8, 4, 32, 32) and hr.min() >= 0
    K, b1, b2, sig = (data[k].double().cpu().numpy() for k in ('K', 'beta1', 'beta2', 'sigma'))
    assert len(set(K)) == 8 and np.allclose(b1, K / 959, rtol=1e-6) and np.allclose(b2, (sig / 959) ** 2, rtol=1e-6)
    assert np.exp(-2.5) <= K.min() and K.max() <= np.exp(3.5)
    r = (lr - hr).reshape(8, -1)
    n = r.shape[1]
    for b in range(8):
        # r = beta1 (k - lambda) + g with lambda = hr / beta1, g ~ N(0, beta2): E r^2 = v = beta1 hr + beta2 per element and, from the
        # Poisson central moments mu2 = lambda, mu4 = lambda + 3 lambda^2, E r^4 = beta1^4 (lambda + 3 lambda^2) + 6 beta1^2 lambda beta2
        # + 3 beta2^2, so Var(r^2) = E r^4 - v^2 = beta1^3 hr + 2 v^2.  The mean of r^2 over the item's n independent elements (the mean
        # of r is known to be 0) has variance sum(Var(r^2)) / n^2.
        h = hr[b].flatten()
        v = b1[b] * h + b2[b]
        got, want = (r[b] ** 2).mean().item(), v.mean().item()
        se = float(torch.sqrt((b1[b] ** 3 * h + 2 * v ** 2).sum()).item()) / n
        print(f"item {b}: K {K[b]:.3f}, sigma {sig[b]:.3f} DN: mean (lr - hr)^2 {got:.4e} vs beta1 mean(hr) + beta2 {want:.4e} ({abs(got - want) / se:.2f} se)")
        assert abs(got - want) <= 5 * se, b
    for b in range(4):                                                                    # the same crop, another slot: independent noise
        c = torch.corrcoef(torch.stack([r[b], r[b + 4]]))[0, 1].item()
        assert abs(c) < 5 / np.sqrt(n), (b, c)
    # evaluation: item k is the same in every pass
    first = [tr.src_eval.item(k) for k in range(len(tr.dst_eval))]
    m1 = dict(tr.eval(-1))
    second = [tr.src_eval.item(k) for k in range(len(tr.dst_eval))]
    m2 = dict(tr.eval(-1))
    assert len(first) == 16
    for k, (p, q) in enumerate(zip(first, second)):                                       # every item, bit for bit
        assert torch.equal(p['lr'], q['lr']) and torch.equal(p['hr'], q['hr']) and not torch.equal(p['lr'], p['hr']), k
        assert p['pattern'] == q['pattern'] == k % 4 and torch.equal(p['K'], q['K']) and torch.equal(p['sigma'], q['sigma'])
    assert len({float((p['lr'] - p['hr']).double().sum()) for p in first}) == 16          # ... and each its own noise
    assert m1 == m2 and len(m1) == 16                                                     # the forward has no atomics: the same metrics
    a = first[3]
    # --synth-noise moves the evaluation level
    tr2 = TA.AWGN_Trainer(['-f', rf, '-m', 'eval', '--synth-noise', '0.5,1'])
    assert (tr2.dst_eval.p['K'], tr2.dst_eval.p['sigma']) == (0.5, 1.0)
    c = tr2.src_eval.item(3)
    assert torch.equal(c['hr'], a['hr']) and (c['lr'] - c['hr']).std() < (a['lr'] - a['hr']).std()
    # a guided architecture would get sigma in DN as its AWGN guidance: refused at construction
    rfg, _ = _pg_runfile(tmp_path, "pg_guided.yml", arch="GRU_5to50_norm_mix.yml")
    with pytest.raises(ValueError, match="guided"):
        TA.AWGN_Trainer(['-f', rfg, '-m', 'train'])


# -- --synth-noise in the full-frame driver --------------------------------------------------------------------------------------
def test_synth_noise_driver(tmp_path, monkeypatch):
    """`YOND_any --synthetic 3 --synth-noise 4,6` on 512 x 768 frames: clean frames in, device noise, the true level and the
    estimator's relative error out; the estimator is as accurate on device-made frames as on host-made ones; without the flag the
    driver sees the frames and gives the metrics it gave before."""
    import zlib
    import yaml
    from yond_public_amd import YOND_full as Y
    from yond_public_amd import pipeline as P
    from yond_public_amd import synthetic as S
    monkeypatch.chdir(tmp_path)
    H, W, K, SIG = 512, 768, 4.0, 6.0
    cfg = yaml.load(open(os.path.join(ROOT, "runfiles", "YOND", "ANY_simple+full_pre_grumix.yml")).read(), Loader=yaml.FullLoader)
    for sec in ('dst', 'dst_eval', 'dst_test'):
        cfg[sec].update(root_dir=str(tmp_path / "nowhere"), H=H, W=W)
    rf = tmp_path / "any.yml"
    rf.write_text(yaml.dump(cfg))
    drv = Y.YOND_Full(['-f', str(rf), '-m', 'eval', '--synthetic', '3', '--synth-noise', '4,6'])
    assert type(drv.dst_eval).__name__ == 'SyntheticFrames' and drv.dst_eval.clean_only and 'lr' not in drv.dst_eval[0]
    res = drv.eval(-1)
    wp, bl = 1023.0, 63.0
    assert set(res) == {'x1', 'x2'} and len(drv.metrics) == 6
    for ratio in (1, 2):
        red = res[f'x{ratio}']
        assert red['count'] == 3 and 0 <= red['rel_err_K_iter0'] < 1 and 0 <= red['rel_err_sigma_iter0'] < 1
        drv.dst_eval.change_eval_ratio(ratio=ratio)
        for k in range(3):
            item = drv.dst_eval[k]
            m = drv.metrics[item['name']]
            assert m['true'] == (K * ratio, SIG * ratio) and 1 <= len(m['rel_err']) <= 2 and len(m['psnr']) >= 1
            assert all(len(e) == 2 and np.isfinite(e).all() for e in m['rel_err'])
            clean = torch.from_numpy(item['hr']).to(DEV)
            noisy = PG.add_pg_noise(clean, K, SIG, wp - bl, zlib.crc32(item['name'].encode()), [0], exposure=1.0 / ratio)
            ps, _ = P.block_metrics(noisy, clean.clamp(0, 1), bh=H, bw=W)
            print(f"{item['name']}: noisy {float(np.mean(ps)):.2f} dB -> rounds {m['psnr']}, rel err (K, sigma) per round {m['rel_err']}")
            assert m['psnr'][-1] > float(np.mean(ps))
    red1 = np.mean([drv.metrics[drv.dst_eval[k]['name']]['rel_err'][0][0] for k in range(3)])
    assert abs(red1 - res['x2']['rel_err_K_iter0']) < 1e-12

    # SIGMA = 0 (shot noise only) has no relative sigma error: None per frame, no mean in the sweep, nothing non-finite
    shot = Y.YOND_Full(['-f', str(rf), '-m', 'eval', '--synthetic', '1', '--synth-noise', '4,0'])
    res_shot = shot.eval(-1)
    for m in shot.metrics.values():
        assert m['true'][1] == 0 and all(e[1] is None and np.isfinite(e[0]) for e in m['rel_err'])
    assert all('rel_err_sigma_iter0' not in r and np.isfinite(r['rel_err_K_iter0']) for r in res_shot.values())

    # the estimator on device-made frames vs host-made frames of the same scene, level and exposure
    clean = torch.from_numpy(S.synth_clean(H, W).astype(np.float32)).to(DEV)
    p = P.default_params()

    def k_est(frame):
        return float(P.IterDenoise(frame, drv.net, drv.arch, drv.pipe, p=dict(p), device=DEV)['params'][0][0])
    dev_err = max(abs(k_est(PG.add_pg_noise(clean, K, SIG, p['scale'], 1997, [slot])) - K) for slot in range(8))
    host_err = max(abs(k_est(torch.from_numpy(S.synth_noisy(H, W, K, SIG, idx, clip=False)[0]).to(DEV)) - K) for idx in range(8))
    print(f"round-1 max |K_est - K| over 8 frames: device noise {dev_err:.4f}, host noise {host_err:.4f} (K = {K})")
    assert dev_err <= 3 * host_err

    # without the flag: the host-drawn frames and the metrics of the one-frame-at-a-time path, computed here
    plain = Y.YOND_Full(['-f', str(rf), '-m', 'eval', '--synthetic', '3'])
    assert plain.synth_noise is None and not plain.dst_eval.clean_only
    res0 = plain.eval(-1)
    for ratio in (1, 2):
        plain.dst_eval.change_eval_ratio(ratio=ratio)
        for k in range(3):
            item = plain.dst_eval[k]
            rng = np.random.default_rng(4000 + k)                 # SyntheticFrames' host draw, restated
            c = (S.synth_clean(H, W) * (0.6 / ratio)).astype(np.float32)
            want = ((rng.poisson(c * 959.0 / 2.0) * 2.0 + rng.normal(0.0, 8.0, c.shape)) / 959.0 * ratio).astype(np.float32)
            assert np.array_equal(item['lr'], want) and np.array_equal(item['hr'], (c * ratio).astype(np.float32))
            m = plain.metrics[item['name']]
            assert set(m) == {'psnr', 'ssim', 'reg'}
            q = dict(plain.pipe, wp=wp, bl=bl, ratio=ratio, gain=1, sigma=0, scale=(wp - bl) / ratio)
            ref = P.IterDenoise(torch.from_numpy(item['lr']).to(DEV), plain.net, plain.arch, plain.pipe, p=q, device=DEV)
            hr = torch.from_numpy(item['hr']).to(DEV)
            for it, dn in enumerate(ref['raw_dns']):
                ps, ss = P.block_metrics(dn, hr.clamp(0, 1), bh=H, bw=W)
                assert abs(float(np.mean(ps)) - m['psnr'][it]) < 2e-3       # (the bound between the two paths in tests/test_hip_eval.py)
    assert all('rel_err_K_iter0' not in r for r in res0.values())
