"""GPU: yond_render_srgb (csrc/isp.hip) and yond_block_metrics_rgb8 (csrc/metrics.hip) against tests/golden/isp.npz (the reference's
process_sidd_image / FastISP / calculate_ssim around the restated demosaic) and tests/isp_model.py, the host wrappers and the
driver's --fig.

The code rule: a kernel code equals the golden (or the model) code, or differs by one where -- and only where -- the model's x lies
within 2^-48 t_k of the threshold t_k between the two (isp_model.in_band): there NumPy's own array and scalar pow disagree.
The float rule: ulp32 / 2 + 1e-12 of the model's float64 value (tests/vst_model.py); where x < 2^-40 (cancellation noise under a pow
of unbounded slope) 1e-6 absolute.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import isp_model as M
import vst_model as V

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNFILE = os.path.join(ROOT, "runfiles", "YOND", "SIDD_simple+full_pre_grumix.yml")
TAIL = 4096
U8_CANARY = 0xA5
BAND_CAP = 0.005
SAT_CST = np.array([[0.9142, -0.3268, -0.0871], [-0.4537, 1.3009, 0.1652], [-0.0913, 0.2446, 0.6104]])      # cam2rgb diagonal 1.6 .. 2.1: clips
WB = np.array([[0.5234375, 1.0, 0.6171875]])
BGGR = [[3, 2], [2, 1]]


@pytest.fixture(scope="module")
def g(golden):
    return golden("isp")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def render(frame, H, W, flips, layout, gains, ccm, mode, order=None, gamma=None, expect=0):
    """One yond_render_srgb call with each output at the front of a canary-filled allocation.  -> (u8 [H][W][3] or None, f32 or None)."""
    from yond_public_amd import _lib as L, isp
    lib = L.load()
    n = H * W * 3 if H > 0 and W > 0 else 0
    u8 = torch.full((n + TAIL,), U8_CANARY, dtype=torch.uint8, device=DEV) if order is not None else None
    f32 = torch.full((n + TAIL,), float('nan'), dtype=torch.float32, device=DEV) if gamma is not None else None
    fr = dev(np.asarray(frame, np.float32))
    thr = dev(isp.threshold_table())
    rc = lib.yond_render_srgb(L.ptr(fr), H, W, int(flips[0]), int(flips[1]), layout, (C.c_double * 4)(*[float(v) for v in gains]),
                              (C.c_double * 9)(*np.asarray(ccm, np.float64).reshape(9)), mode, L.ptr(thr), L.ptr(u8),
                              isp.ORDERS.get(order, 0), L.ptr(f32), float(gamma or 0.0), L.stream())
    torch.cuda.synchronize()
    assert rc == expect, f"yond_render_srgb returned {rc}, expected {expect}"
    if expect != 0:                                                             # refused: nothing written
        assert u8 is None or bool((u8 == U8_CANARY).all())
        assert f32 is None or bool(torch.isnan(f32).all())
        return None, None
    if u8 is not None:
        assert bool((u8[n:] == U8_CANARY).all()), "the u8 output's tail was written"
        u8 = u8[:n].reshape(H, W, 3).cpu().numpy()
    if f32 is not None:
        assert bool(torch.isnan(f32[n:]).all()), "the float output's tail was written"
        f32 = f32[:n].reshape(H, W, 3).cpu().numpy()
    return u8, f32


def sidd_args(pattern, wb, cst):
    wb = np.asarray(wb, np.float64).reshape(-1)
    return M.flips_of(pattern), (1 / wb[0], 1 / wb[1], 1 / wb[1], 1 / wb[2]), M.cam2rgb(cst)


def check_float(got, x, inv_gamma, what):
    want = x ** inv_gamma
    tiny = x < 2.0 ** -40
    assert got.dtype == np.float32 and np.isfinite(got).all()
    if tiny.any():
        assert np.abs(got[tiny].astype(np.float64) - want[tiny]).max() <= 1e-6, what
    V.ulp_check(np.where(tiny, want.astype(np.float32), got), want, 1e-12, what)


def test_goldens_codes_and_orders(g):
    for c in g["sidd_cases"]:
        frame, pattern, want = g[c + "_frame"], g[c + "_pattern"], g[c + "_bgr"]
        _, x = M.render_sidd(frame, pattern, g["wb"], g["cst"])
        share = float(M.in_band(x).mean())                                      # from the model alone, before the kernel is looked at
        assert share <= BAND_CAP, f"{c}: {share:.4%} of the elements lie in a threshold's band"
        if c.startswith("crop_"):
            assert share == 0.0, f"{c} holds no white and must have no element in the band"
        flips, gains, ccm = sidd_args(pattern, g["wb"], g["cst"])
        H, W = frame.shape
        bgr, _ = render(frame, H, W, flips, 0, gains, ccm, M.SIDD, order='bgr')
        rgb, _ = render(frame, H, W, flips, 0, gains, ccm, M.SIDD, order='rgb')
        n = M.check_codes(bgr, want, x[..., ::-1], c)
        np.testing.assert_array_equal(rgb, bgr[..., ::-1])
        print(f"[isp] {c} {H}x{W}: {n} of {want.size} codes differ from the golden inside the band ({share:.3%} in the band)")


def test_host_wrappers_on_the_goldens(g, tmp_path):
    """isp.render_sidd / utils.process_sidd_image: the reference's signature and return value, and the PNG holds RGB."""
    from PIL import Image
    from yond_public_amd import isp
    from yond_public_amd.utils import process_sidd_image
    c = "scene_gbrg"
    frame, pattern, want = g[c + "_frame"], g[c + "_pattern"].tolist(), g[c + "_bgr"]
    _, x = M.render_sidd(frame, pattern, g["wb"], g["cst"])
    path = str(tmp_path / "scene.png")
    out = process_sidd_image(frame, pattern, g["wb"], g["cst"], save_file_rgb=path)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == want.shape
    M.check_codes(out, want, x[..., ::-1], "process_sidd_image")
    png = np.asarray(Image.open(path))
    assert png.shape == out.shape and png.dtype == np.uint8
    np.testing.assert_array_equal(png, out[:, :, ::-1])
    dev_rgb = isp.render_sidd(dev(frame), pattern, g["wb"], g["cst"], order='rgb')
    assert dev_rgb.is_cuda and dev_rgb.dtype == torch.uint8
    np.testing.assert_array_equal(dev_rgb.cpu().numpy(), out[:, :, ::-1])
    with pytest.raises(ValueError):
        isp.render_sidd(dev(frame), [[1, 2], [3, 2]], g["wb"], g["cst"])


def test_fastisp_float_form(g):
    from yond_public_amd.utils import FastISP
    img4c = g["fast_img4c"]
    for c in g["fast_cases"]:
        wb, ccm = (g["fast_wb"], g["fast_ccm"]) if c == "fast_given" else (None, None)
        y, x = M.fast_isp(img4c, wb, ccm)
        gains = (2.0, 1.0, 1.0, 2.0) if wb is None else (wb[0], 1.0, 1.0, wb[2])
        _, got = render(img4c, 32, 48, (0, 0), 1, gains, M.SONY_CCM if ccm is None else ccm, M.FAST, gamma=2.2)
        check_float(got, x, 1 / 2.2, c)
        np.testing.assert_allclose(got, g[c + "_rgb"], rtol=0, atol=2.0 ** -24 + 1e-6)          # and the golden itself (4 float64 ulp from the model)
        out = FastISP(torch.from_numpy(img4c)[None], wb, ccm)                                   # a tensor whose [0] is taken
        assert isinstance(out, np.ndarray) and out.shape == (32, 48, 3)
        np.testing.assert_array_equal(out, got)
    _, got = render(img4c, 32, 48, (0, 0), 1, (1.5, 1.0, 1.0, 1.25), M.SONY_CCM, M.FAST, gamma=1.8)   # another gamma
    check_float(got, M.linear(M.unpack4(img4c), (1.5, 1.0, 1.0, 1.25), M.SONY_CCM, M.FAST), 1 / 1.8, "gamma 1.8")


SHAPES = [(2, 2), (2, 130), (66, 2), (34, 66), (64, 256), (18, 136)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_shapes_against_the_model(H, W):
    """Both flips on, a saturating colour matrix, inputs beyond [0, 1]: tile edges (16 x 128), one-quad rows and columns, the mirror at all
    four borders, W % 4 == 2 (no 16-byte row loads, odd rows off the 4-byte store grid) and W % 4 == 0.  Codes and the float form in ONE call."""
    rng = np.random.default_rng(1000 * H + W)
    frame = rng.uniform(-0.2, 1.4, (H, W)).astype(np.float32)
    flips, gains, ccm = sidd_args(BGGR, WB, SAT_CST)
    assert flips == (True, True)
    x = M.linear(frame, gains, ccm, M.SIDD, True, True)
    u8, f32 = render(frame, H, W, flips, 0, gains, ccm, M.SIDD, order='rgb', gamma=2.2)
    n = M.check_codes(u8, M.codes_of(x), x, f"{H}x{W} codes")
    check_float(f32, x, 1 / 2.2, f"{H}x{W} float")
    print(f"[isp] {H}x{W}: {n} codes differ from the model inside the band, {int(M.in_band(x).sum())} elements in the band")
    if (H, W) == (34, 66):                                                       # every single flip too
        for fl, pat in (((False, False), [[1, 2], [2, 3]]), ((True, False), [[2, 1], [3, 2]]), ((False, True), [[2, 3], [1, 2]])):
            xx = M.linear(frame, gains, ccm, M.SIDD, *fl)
            got, _ = render(frame, H, W, M.flips_of(pat), 0, gains, ccm, M.SIDD, order='bgr')
            M.check_codes(got, M.codes_of(xx)[..., ::-1], xx[..., ::-1], f"flips {fl}")


@pytest.mark.parametrize("value", [1.3, -0.1])
def test_saturated_frames(value):
    H, W = 34, 66
    frame = np.full((H, W), value, np.float32)
    flips, gains, ccm = sidd_args(BGGR, WB, SAT_CST)
    x = M.linear(frame, gains, ccm, M.SIDD, True, True)
    u8, f32 = render(frame, H, W, flips, 0, gains, ccm, M.SIDD, order='bgr', gamma=2.2)
    M.check_codes(u8, M.codes_of(x)[..., ::-1], x[..., ::-1], f"all {value}")
    check_float(f32, x, 1 / 2.2, f"all {value}")
    assert (u8 >= 254).all() if value > 1 else (u8 == 0).all()                   # white renders as 254 or 255 by the row sum of cam2rgb


def test_refusals_write_nothing():
    flips, gains, ccm = sidd_args(BGGR, WB, SAT_CST)
    frame = np.zeros((8, 8), np.float32)
    for H, W in ((7, 8), (8, 7), (0, 8), (8, 0)):
        render(frame, H, W, flips, 0, gains, ccm, M.SIDD, order='bgr', gamma=2.2, expect=-1)
    render(frame, 8, 8, flips, 0, gains, ccm, M.SIDD, expect=-1)                # both outputs null
    render(frame, 8, 8, flips, 1, gains, ccm, M.FAST, order='bgr', expect=-1)   # flips with the packed layout
    render(frame, 8, 8, (0, 0), 2, gains, ccm, M.SIDD, order='bgr', expect=-1)  # unknown layout


# ---------------------------------------------------------------------------------------------------------------------------
# yond_block_metrics_rgb8
# ---------------------------------------------------------------------------------------------------------------------------
SSIM_TOL, PSNR_TOL = 1e-9, 1e-6           # the bounds of test_block_metrics_vs_oracle: the inputs are exact integers <= 255, so the reasoning
#                                           at tests/test_hip_vst_edges.py (C1, C2 bound the denominators; 1e-10 of rounding per moment) holds


def run_rgb8(dn, hr, bh, bw, expect=0):
    from yond_public_amd import _lib as L
    lib = L.load()
    H, W = dn.shape[:2]
    nt = lib.yond_block_metrics_tiles(bh, bw)
    n = (H // bh) * (W // bw) * max(nt, 1) * 6
    out = torch.full((n + TAIL,), float('nan'), dtype=torch.float64, device=DEV)
    a, b = dev(dn), dev(hr)
    rc = lib.yond_block_metrics_rgb8(L.ptr(a), L.ptr(b), H, W, bh, bw, L.ptr(out), L.stream())
    torch.cuda.synchronize()
    assert rc == expect
    if expect != 0:
        assert bool(torch.isnan(out).all())
        return None
    assert bool(torch.isnan(out[n:]).all()) and bool(torch.isfinite(out[:n]).all())
    return out[:n].reshape(-1, nt, 3, 2).cpu().numpy()


def test_block_metrics_rgb8_on_the_metrics_pair(g):
    from yond_public_amd import isp
    dn, hr = g["metrics_dn_bgr"], g["metrics_hr_bgr"]
    assert dn.shape == (64, 512, 3) and (dn != hr).any()
    psnr, ssim = isp.block_metrics_rgb(dev(dn), dev(hr), 64, 64)
    print("[isp] psnr_rgb", psnr, "ssim_rgb", ssim)
    np.testing.assert_allclose(psnr, g["metrics_psnr_rgb"], rtol=0, atol=PSNR_TOL)
    np.testing.assert_allclose(ssim, g["metrics_ssim_rgb"], rtol=0, atol=SSIM_TOL)
    s = run_rgb8(dn, hr, 64, 64)                                                # the raw sums: the squared code errors are exact integers
    se = ((dn.astype(np.int64) - hr.astype(np.int64)) ** 2).reshape(64, 8, 64, 3).sum(axis=(0, 2))
    np.testing.assert_array_equal(s[..., 0].sum(axis=1), se.astype(np.float64))
    # the kernel's renders of the same pair score the same to the band's one-code differences: here, exactly the goldens' images
    rd = isp.render_sidd(g["metrics_dn"], isp.RGGB, g["wb"], g["cst"], order='bgr')
    _, x = M.render_sidd(g["metrics_dn"], isp.RGGB, g["wb"], g["cst"])
    M.check_codes(rd.cpu().numpy(), dn, x[..., ::-1], "metrics pair render")


@pytest.mark.parametrize("bh,bw", [(11, 11), (40, 72)])
def test_block_metrics_rgb8_small_and_partial_tiles(bh, bw):
    import yond_oracle as O
    from yond_public_amd import isp
    rng = np.random.default_rng(bh * 100 + bw)
    hr = rng.integers(0, 256, (2 * bh, 3 * bw, 3)).astype(np.uint8)
    dn = np.clip(hr.astype(np.int64) + rng.integers(-9, 10, hr.shape), 0, 255).astype(np.uint8)
    psnr, ssim = isp.block_metrics_rgb(dev(dn), dev(hr), bh, bw)
    run_rgb8(dn, hr, bh, bw)                                                    # (the canary)
    k = 0
    for by in range(2):
        for bx in range(3):
            a, b = dn[by * bh:(by + 1) * bh, bx * bw:(bx + 1) * bw], hr[by * bh:(by + 1) * bh, bx * bw:(bx + 1) * bw]
            assert abs(psnr[k] - O.psnr(a, b, 255.0)) <= PSNR_TOL
            assert abs(ssim[k] - np.mean([O.ssim(a[..., c], b[..., c]) for c in range(3)])) <= SSIM_TOL
            k += 1


def test_block_metrics_rgb8_refusals():
    from yond_public_amd import _lib as L, isp
    img = np.zeros((20, 20, 3), np.uint8)
    run_rgb8(img, img, 10, 10, expect=-1)
    run_rgb8(img, img, 20, 10, expect=-1)
    run_rgb8(img, img, 12, 20, expect=-1)                                       # H % bh != 0
    with pytest.raises(L.YondHipError):
        isp.block_metrics_rgb(dev(img), dev(img), 10, 10)


# ---------------------------------------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------------------------------------
def test_driver_fig(tmp_path, monkeypatch):
    from PIL import Image
    from yond_public_amd import YOND_SIDD as Y
    monkeypatch.chdir(tmp_path)
    red = Y.main(['-f', RUNFILE, '-m', 'eval', '--synthetic', '2', '--fig', '--group', '1'])
    t = Y.main.trainer
    n_it = t.pipe['max_iter'] + 1
    assert red['count'] == 2 and np.isfinite(red['psnr_rgb_last']) and np.isfinite(red['ssim_rgb_last'])
    assert 0 < red['ssim_rgb_last'] <= 1 and 5 < red['psnr_rgb_last'] < 100
    last_p, last_s = [], []
    for k in range(2):
        name = t.dst_eval[k]['name']
        m = t.metrics[name]
        assert len(m['psnr_rgb']) == len(m['psnr']) == n_it and len(m['ssim_rgb']) == n_it     # one entry per round
        last_p.append(m['psnr_rgb'][-1]); last_s.append(m['ssim_rgb'][-1])
        for kind in ['noisy', 'gt'] + [str(it) for it in range(n_it)]:
            img = np.asarray(Image.open(os.path.join(t.sample_dir, f'{name}_{kind}.png')))
            assert img.shape == (256, 8192, 3) and img.dtype == np.uint8
    assert abs(red['psnr_rgb_last'] - np.mean(last_p)) < 1e-9 and abs(red['ssim_rgb_last'] - np.mean(last_s)) < 1e-12
    assert abs(red[f'psnr_rgb_iter{n_it - 1}'] - np.mean(last_p)) < 1e-9
    log = open(t.logfile).read()
    assert log.count('PSNR(sRGB)=') == 2 + n_it + 1                              # per image, per iteration, Iter_last


def test_driver_without_fig_is_todays(tmp_path, monkeypatch):
    from yond_public_amd import YOND_SIDD as Y
    monkeypatch.chdir(tmp_path)
    red = Y.main(['-f', RUNFILE, '-m', 'eval', '--synthetic', '1', '--group', '1'])
    t = Y.main.trainer
    n_it = t.pipe['max_iter'] + 1
    assert sorted(red) == sorted(['count', 'psnr_last', 'ssim_last'] + [f'{k}_iter{it}' for k in ('psnr', 'ssim') for it in range(n_it)])
    assert all(sorted(m) == ['psnr', 'reg', 'ssim'] for m in t.metrics.values())
    assert not os.path.exists(t.sample_dir) and 'sRGB' not in open(t.logfile).read()
