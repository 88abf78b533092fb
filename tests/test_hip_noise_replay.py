"""GPU: the three noise generators replayed element by element.  yond_pg_noise_f32, yond_camera_noise_f32 and yond_img2raw_f32 are
launched with power-of-two scales so that the stored value IS one draw, and each draw is held to the model of tests/noise_replay.py:
the Philox counter, key and tag, the word that feeds each draw, its bits.  Counts are held to the host build of the same sampler
source: equal on every element that does not hang on the last bits of logf / expf / log1pf (NR.robust_mask), the others at most 0.1 %;
above 2^23, where the count is a rounded normal, every element within 1.  Normals and Tukey-lambda variates are held to the float64
model within NR.TOL_FACTOR x the host build's own deviation from it (NR.HOST_DEV, measured in tests/test_noise_replay_model.py,
never on the device).  img2raw's hr is held to the gather model on the shapes, rotations and highlights its fixtures miss.
Each test prints `[replay]` lines; profiles/noise_replay_report.txt keeps one run."""
import numpy as np
import pytest
import torch

import noise_replay as NR
import pgnoise_stats as PS
from yond_public_amd import camnoise as CN
from yond_public_amd import img2raw as I
from yond_public_amd import pgnoise as PG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEY, CAM_KEY = 20261018, 20261019
BETA1 = 2.0 ** -6
N = 2 ** 16
CAM_LAMS = (-0.26, -0.026, 0.0, 0.015, 0.102)
TOL = {k: NR.TOL_FACTOR * v for k, v in NR.HOST_DEV.items()}
HALF_ULP = 2.0 ** -24


def _np(t):
    return t.detach().double().cpu().numpy()


def _ladder():
    return PS.ladder(PG.SWITCH_LAMBDAS)


# -- pg ---------------------------------------------------------------------------------------------------------------------------
def _pg_counts(lam_per_element, slot, out=None, clean=None):
    """beta1 = 2^-6, sigma_n = 0, e = 1: the stored value is k beta1 exactly."""
    if clean is None:
        clean = torch.from_numpy((np.asarray(lam_per_element, np.float32) * np.float32(BETA1))).to(DEV)
    return _np(PG.add_pg_noise(clean, BETA1, 0.0, 1.0, KEY, [slot], out=out)) / BETA1


def test_pg_counts_per_ladder_lambda():
    bad, worst = [], 0.0
    for slot, lam in enumerate(_ladder()):
        k = _pg_counts(np.full(N, lam, np.float32), slot)
        mask, host = NR.robust_mask(KEY, slot, 0, N, [lam])
        fails = NR.compare_counts(k, host, mask, lam)
        normal = lam > PG.SWITCH_LAMBDAS[1]
        print(f"[replay] gpu pg lambda {lam:14.6f}: fragile {int((~mask).sum()):3d} of {N} ({(~mask).mean():.4%}), device != host at "
              f"{int((k != host).sum())} (max |dk| {np.abs(k - host).max():.0f})" + ("   FAIL: " + "; ".join(fails) if fails else ""))
        bad += [f"lambda {lam}: {f}" for f in fails]
        if not normal:
            worst = max(worst, float((~mask).mean()))
    assert worst <= NR.FRAGILE_SHARE_MAX
    assert not bad, bad


def test_pg_normal_is_the_models():
    """beta1 = 0, sigma_n = 2^-3, clean = 0: the stored value is z / 8 exactly."""
    for slot in (0, 7):
        out = PG.add_pg_noise(torch.zeros(N, device=DEV), 0.0, 0.125, 1.0, KEY, [slot])
        z = _np(out) / 0.125
        want = NR.pg_z(KEY, slot, np.arange(N, dtype=np.uint64))
        print(f"[replay] gpu pg z, slot {slot}: max |device - model| {NR.deviation(z, want):.3e} (tolerance {TOL['z']:.1e})")
        fails = NR.compare_values(z, want, TOL["z"], what="z")
        assert not fails, fails


def test_pg_mixed_launch_and_unaligned_view():
    lams = np.array(_ladder(), np.float32)
    assert set(np.digitize(lams, PG.SWITCH_LAMBDAS)) == {0, 1, 2} and lams.size < 64          # every regime inside every wavefront
    lam = lams[np.arange(N) % lams.size]
    mask, host = NR.robust_mask(KEY, 0, 0, N, lams)
    k = _pg_counts(lam, 0)
    fails = NR.compare_counts(k, host, mask, lam)
    print(f"[replay] gpu pg mixed ladder: fragile {int((~mask).sum())} of {N}, device != host at {int((k != host).sum())}"
          + ("   FAIL: " + "; ".join(fails) if fails else ""))
    assert not fails, fails
    # one float into a buffer, in and out: the head / tail units replay with the element's index in the item, not in the buffer
    for n in (4099, 4100, 4101, 4102, 2, 3):
        buf_in, buf_out = torch.zeros(n + 8, device=DEV), torch.full((n + 8,), -7.0, device=DEV)
        buf_in[1:n + 1] = torch.from_numpy(lam[:n] * np.float32(BETA1)).to(DEV)
        kv = _pg_counts(None, 0, out=buf_out[1:n + 1], clean=buf_in[1:n + 1])
        fails = NR.compare_counts(kv, host[:n], mask[:n], lam[:n])
        assert not fails, (n, fails)
        assert np.array_equal(kv, k[:n]), n
        assert buf_out[0] == -7.0 and (buf_out[n + 1:] == -7.0).all()
    print("[replay] gpu pg unaligned views of 4099, 4100, 4101, 4102, 2, 3 elements: equal to the aligned launch and to the host")


# -- camnoise ---------------------------------------------------------------------------------------------------------------------
def _cam(clean, slot, layout=CN.LAYOUT_PLANAR, row_len=None, K=0.0, sig_read=0.0, **kw):
    return _np(CN.launch(clean, CN.plan(1, K, sig_read, 1.0, CAM_KEY, [slot], **kw), layout=layout, row_len=row_len))


def test_cam_quantisation_uniform_is_word_2_exactly():
    """q_step = 1 alone on clean = 0: 0 + (0 z_row + 1 uq + 0) / 1 -- 23 known bits of word 2 per element."""
    for slot in (0, 3):
        got = _cam(torch.zeros(N, device=DEV), slot, q_step=1.0)
        want = NR.cam_draw(CAM_KEY, slot, np.arange(N, dtype=np.uint64), 0.0)[1]
        print(f"[replay] gpu cam uq, slot {slot}: {int((got != want).sum())} of {N} differ from the model (exact)")
        assert np.array_equal(got, want)


@pytest.mark.parametrize("lam", CAM_LAMS)
def test_cam_tukey_lambda_is_the_models(lam):
    """sig_read = 1 with the Tukey-lambda flag alone on clean = 0: the stored value is the variate."""
    slot = CAM_LAMS.index(lam)
    got = _cam(torch.zeros(N, device=DEV), slot, sig_read=1.0, lam=lam, tukey=True)
    want = NR.cam_draw(CAM_KEY, slot, np.arange(N, dtype=np.uint64), lam)[0]
    print(f"[replay] gpu cam tl lam {lam:7.3f}: max |device - model| / max(1, |model|) {NR.deviation(got, want, 'rel'):.3e} "
          f"(tolerance {TOL['tl']:.1e}), |tl| up to {np.abs(want).max():.1f}")
    fails = NR.compare_values(got, want, TOL["tl"], "rel", what="tl")
    assert not fails, fails
    nz = want != 0
    assert np.array_equal(np.sign(got[nz]), np.sign(want[nz]))                                 # word 1 bit 0


def test_cam_gaussian_shot_normal_is_words_3_1():
    """Gaussian shot approximation alone on clean = 0: y = 0, the variance floor 1e-10 stands, the stored value is
    fl(zs sqrtf(1e-10f)) beta1 with beta1 = 2^-6: one rounding, 2^-24 |zs| after the division by the two constants."""
    s = float(np.sqrt(np.float32(1e-10)))
    for slot in (0, 4):
        got = _cam(torch.zeros(N, device=DEV), slot, K=BETA1, poisson=False) / (BETA1 * s)
        want = NR.cam_draw(CAM_KEY, slot, np.arange(N, dtype=np.uint64), 0.0)[2]
        print(f"[replay] gpu cam zs, slot {slot}: max |device - model| {NR.deviation(got, want):.3e} (tolerance {TOL['zs']:.1e} + 2^-24 |zs|)")
        fails = NR.compare_values(got, want, TOL["zs"] + HALF_ULP * np.abs(want), what="zs")
        assert not fails, fails


@pytest.mark.parametrize("layout, shape", [(CN.LAYOUT_PLANAR, (4, 6, 20)), (CN.LAYOUT_BAYER, (12, 20)), (CN.LAYOUT_BAYER, (5, 28)),
                                           (CN.LAYOUT_BAYER, (1024, 4)), (CN.LAYOUT_BAYER, (1024, 6))])
def test_cam_row_normal_is_the_rows(layout, shape):
    """sig_row = 2^-3 alone on clean = 0: every element of row r = index / row_len stores z_row(r) / 8."""
    n, w = int(np.prod(shape)), shape[-1]
    got = _cam(torch.zeros(shape, device=DEV), 2, layout=layout, sig_row=0.125).reshape(-1) / 0.125
    rows = NR.cam_rows(n, w)
    want = NR.cam_row_normal(CAM_KEY, 2, rows)
    print(f"[replay] gpu cam row, layout {layout} {shape}: max |device - model| {NR.deviation(got, want):.3e} (tolerance {TOL['row']:.1e})")
    fails = NR.compare_values(got, want, TOL["row"], what="row")
    assert not fails, fails
    per_row = got.reshape(-1, w)
    assert np.array_equal(per_row, np.broadcast_to(per_row[:, :1], per_row.shape))             # one float per row


def test_cam_everything_on_is_the_sum_of_the_replayed_terms():
    """Poisson shot at lambda 50, Tukey-lambda read, row, quantisation and bias on one Bayer frame of 64 x 28, e = m = 1: the kernel's
    fl(fl(k beta1 + read) + fl(fl(fl(srow z_row + q uq) + b))) against the float64 sum of the model's terms, with the host build's
    count.  Tolerance: each float64 term's own, scaled, plus four float32 roundings of partial sums no larger than sum |term|."""
    H, W, slot, lam_p, lam_t = 64, 28, 6, 50.0, -0.026
    sr, srow, q = 2.0 ** -4, 2.0 ** -3, 2.0 ** -10
    bias = np.array([2.0 ** -5, -2.0 ** -6, 2.0 ** -7, 0.0])
    n = H * W
    clean = torch.full((H, W), float(np.float32(lam_p) * np.float32(BETA1)), device=DEV)
    got = _cam(clean, slot, layout=CN.LAYOUT_BAYER, K=BETA1, sig_read=sr, lam=lam_t, tukey=True, sig_row=srow, q_step=q, bias=bias).reshape(-1)
    idx = np.arange(n, dtype=np.uint64)
    mask, k = NR.robust_mask(CAM_KEY, slot, 0, n, [lam_p])
    tl, uq, _ = NR.cam_draw(CAM_KEY, slot, idx, lam_t)
    rows = NR.cam_rows(n, W)
    zrow = NR.cam_row_normal(CAM_KEY, slot, rows)
    b = bias[2 * (rows & 1) + (np.arange(n) % W & 1)]
    terms = [k.astype(np.float64) * BETA1, sr * tl, srow * zrow, q * uq, b]
    want = sum(terms)
    tol = sr * TOL["tl"] * np.maximum(1.0, np.abs(tl)) + srow * TOL["row"] + 4 * HALF_ULP * sum(np.abs(t) for t in terms)
    assert (~mask).mean() <= NR.FRAGILE_SHARE_MAX
    print(f"[replay] gpu cam all terms: max |device - model sum| {NR.deviation(got[mask], want[mask]):.3e} (tolerance {tol.min():.1e} .. "
          f"{tol.max():.1e}), fragile {int((~mask).sum())} of {n}")
    fails = NR.compare_values(got[mask], want[mask], tol[mask], what="sum of terms")
    assert not fails, fails


# -- img2raw ----------------------------------------------------------------------------------------------------------------------
def _cache(tmp_path, crops, name):
    d = tmp_path / name
    d.mkdir()
    for i, c in enumerate(crops):
        np.save(d / f"{i:03d}.npy", c)
    return I.CropCache(sorted(str(p) for p in d.glob("*.npy")), DEV)


def _crop(rng, H, W, dtype, lo=0.0):
    top = np.iinfo(dtype).max
    return rng.integers(int(lo * top), top + 1, (H, W, 3)).astype(dtype)


def _table(dtype):
    return I.curve(dtype, 255. if dtype == np.uint8 else 65535., DEV)


@pytest.mark.parametrize("H, W", [(32, 48), (6, 10)])
def test_img2raw_normals_are_the_groups(tmp_path, H, W):
    """clip off, sigma = 2^-3: (lr - hr) / sigma is the group's four normals, up to the one rounding of hr + z sigma."""
    rng = np.random.default_rng(3)
    sigma = 0.125
    cache = _cache(tmp_path, [_crop(rng, H, W, np.uint8)], "c")
    keys, slots = [7, 7, 20261018, 20261018], [0, 5, 0, 5]
    p = I.plan(cache.offsets([0, 0, 0, 0]), [I.eval_meta(1)] * 4, [0] * 4, [sigma] * 4, 0, slots)
    p["key"] = np.array(keys, np.uint32)
    hr, lr, _ = I.launch(cache, _table(np.uint8), p, pattern=0, clip=False)
    plane = (H // 2) * (W // 2)
    z = (_np(lr) - _np(hr)).reshape(4, -1) / sigma
    for b in range(4):
        want = NR.img2raw_normals(keys[b], slots[b], plane).reshape(-1)
        tol = TOL["z"] + HALF_ULP * (1.0 + np.abs(want) * sigma) / sigma
        print(f"[replay] gpu img2raw normals {H}x{W} key {keys[b]} slot {slots[b]}: max |device - model| {NR.deviation(z[b], want):.3e} "
              f"(tolerance {tol.min():.1e} .. {tol.max():.1e})")
        fails = NR.compare_values(z[b], want, tol, what="z")
        assert not fails, (b, fails)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("H, W", [(2, 2), (6, 6), (6, 10), (32, 48)])
def test_img2raw_hr_on_the_shapes_the_fixtures_miss(tmp_path, H, W, dtype):
    """Planes of 1, 9, 15 and 384 elements (a group spanning all four channels, groups straddling planes, wo no multiple of 4, two
    workgroups), every rotation given explicitly -- so the odd ones run with H != W."""
    rng = np.random.default_rng(H * 100 + W)
    crop = _crop(rng, H, W, dtype)
    cache = _cache(tmp_path, [crop], "c")
    table = _table(dtype)
    meta = I.eval_meta(H + W)
    worst = 0.0
    for k in range(4):
        p = I.plan(cache.offsets([0]), [meta], [3 - k], [0.0], 1, [0])                        # the patch's own pattern is not looked at
        hr, lr, _ = I.launch(cache, table, p, pattern=k, clip=True)
        want = NR.gather_model(crop, table.cpu().numpy(), meta["rgb2cam"].numpy(), I.gains(meta).numpy(), k)
        assert tuple(hr.shape[1:]) == want.shape == (4, (W if k & 1 else H) // 2, (H if k & 1 else W) // 2)
        assert torch.equal(hr, lr)                                                            # sigma 0
        worst = max(worst, NR.deviation(_np(hr[0]), want))
    print(f"[replay] gpu img2raw hr {H}x{W} {np.dtype(dtype).name}, patterns 0-3: max |device - gather model| {worst:.3e} (bound 2e-6)")
    assert worst <= 2e-6, worst


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_img2raw_hr_highlight_mask(tmp_path, dtype):
    """A bright crop (gray above 0.9) under gains below 1: the mask blends the gain towards 1, partly and fully."""
    rng = np.random.default_rng(9)
    crop = _crop(rng, 6, 10, dtype, lo=0.985)
    crop[0, 0] = np.iinfo(dtype).max
    cache = _cache(tmp_path, [crop], "c")
    table = _table(dtype)
    meta = dict(I.eval_meta(2), rgb_gain=torch.tensor([1.25]), red=torch.tensor([2.0]), blue=torch.tensor([1.8]))
    gain = I.gains(meta).numpy()
    assert gain.max() < 1
    cam = table.cpu().numpy()[crop.astype(np.int64)] @ meta["rgb2cam"].numpy().T
    mask = (np.maximum(cam.mean(-1) - 0.9, 0) / 0.1) ** 2
    assert (mask > 0.01).sum() >= 10 and (mask < 0.99).any() and mask.max() > 0.99
    worst = 0.0
    for k in range(4):
        p = I.plan(cache.offsets([0]), [meta], [k], [0.0], 1, [0])
        hr, _, _ = I.launch(cache, table, p, pattern=k, clip=True)
        want = NR.gather_model(crop, table.cpu().numpy(), meta["rgb2cam"].numpy(), gain, k)
        worst = max(worst, NR.deviation(_np(hr[0]), want))
    print(f"[replay] gpu img2raw hr bright crop {np.dtype(dtype).name}: mask in [{mask.min():.3f}, {mask.max():.3f}], "
          f"max |device - gather model| {worst:.3e} (bound 2e-6)")
    assert worst <= 2e-6, worst


def test_img2raw_offset_outside_the_cache_gives_nan_for_that_patch_only(tmp_path):
    rng = np.random.default_rng(4)
    H, W = 6, 10
    cache = _cache(tmp_path, [_crop(rng, H, W, np.uint8) for _ in range(2)], "c")
    table = _table(np.uint8)
    metas = [I.eval_meta(i) for i in range(4)]
    off = cache.offsets([0, 1, 1, 0])
    good = I.plan(off, metas, [0] * 4, [0.125] * 4, 11, np.arange(4))
    bad = good.copy()
    bad["offset"][1] = cache.buf.numel() - cache.per + 1                                       # the last pixel would lie outside
    bad["offset"][2] = -1
    h0, l0, _ = I.launch(cache, table, good, pattern=0, clip=False)
    h1, l1, s1 = I.launch(cache, table, bad, pattern=0, clip=False)
    for b in (1, 2):
        assert torch.isnan(h1[b]).all() and torch.isnan(l1[b]).all(), b
    for b in (0, 3):
        assert torch.equal(h1[b], h0[b]) and torch.equal(l1[b], l0[b]) and torch.isfinite(l1[b]).all(), b
    assert torch.equal(s1, torch.full((4,), 0.125, device=DEV))
