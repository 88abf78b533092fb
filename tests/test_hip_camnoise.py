"""GPU: yond_camera_noise_f32 (csrc/camnoise.hip) -- the degenerate case against yond_pg_noise_f32 bit for bit, the counter-based contract
(an element's value depends on its item, its index, its clean value and the geometry only), each term of the model on its own (row,
quantisation, bias, Tukey-lambda read noise), the total variance with and without MultiFrameMean, the clip, the edge rules and the
refusals of include/yond_hip.h -- then --camera-noise in the full-frame driver.
A fixed key makes every statistical check deterministic.  Bounds: 5 standard errors of the statistic under the exact law, chi-square at
a 1e-6 tail (tests/camnoise_stats.py, as tests/pgnoise_stats.py)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import camnoise_stats as CS
from yond_public_amd import _lib
from yond_public_amd import camnoise as CN
from yond_public_amd import pgnoise as PG

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
KEY = 20261019
BETA1 = 2.0 ** -6


def _run(clean, slots=(0,), layout=CN.LAYOUT_PLANAR, row_len=None, out=None, K=0.0, sig_read=0.0, **kw):
    """One launch with parameters in the normalised scale (scale 1)."""
    return CN.launch(clean, CN.plan(len(slots), K, sig_read, 1.0, KEY, list(slots), **kw), layout=layout, row_len=row_len, out=out)


def _frames(shape, seed, lo=-0.25, hi=1.25):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand(shape, device=DEV, generator=g) * (hi - lo) + lo


ALL_ON = dict(K=[BETA1, 0.01, 0.003], sig_read=[0.02, 0.05, 0.1], lam=[-0.26, 0.0, 0.102], sig_row=[0.01, 0.02, 0.03], q_step=2.0 ** -10,
              bias=[[0.01, -0.02, 0.03, 0.005]] * 3, exposure=[1.0, 0.01, 0.37], mfm=[1, 4, 2], tukey=[True, True, False],
              poisson=[True, False, True])


def test_degenerate_case_is_the_pg_kernel():
    K, sig, e, slots = [BETA1, 0.01, 0.003], [0.0, 0.02, 0.1], [1.0, 0.01, 0.37], [3, 4, 5]
    clean = _frames((3, 4, 32, 48), 1)
    want = PG.add_pg_noise(clean, K, sig, 1.0, KEY, slots, exposure=e)
    got = _run(clean, slots, K=K, sig_read=sig, exposure=e)
    assert torch.equal(got, want) and not torch.equal(got, clean)
    # a geometry given and unused changes nothing; lam is not looked at
    assert torch.equal(_run(clean, slots, layout=CN.LAYOUT_BAYER, row_len=48, K=K, sig_read=sig, exposure=e, lam=0.102), want)
    # clip [0, 1] where e = 1
    want = PG.add_pg_noise(clean, K, sig, 1.0, KEY, slots, clip=True)
    got = _run(clean, slots, K=K, sig_read=sig, clip=(0.0, 1.0))
    assert torch.equal(got, want) and got.min() == 0 and got.max() == 1
    # n_per_item = 4 * 5 * 7, no geometry term: any shape goes; and a buffer offset by one float
    flat = _frames((140,), 2)
    want = PG.add_pg_noise(flat, 0.01, 0.02, 1.0, KEY, [9], exposure=0.37)
    assert torch.equal(_run(flat, [9], K=0.01, sig_read=0.02, exposure=0.37), want)
    for m in (1, 3, 4, 5, 139):
        assert torch.equal(_run(flat[:m].clone(), [9], K=0.01, sig_read=0.02, exposure=0.37), want[:m]), m
    buf_in, buf_out = torch.zeros(148, device=DEV), torch.full((148,), -7.0, device=DEV)
    buf_in[1:141] = flat
    for cin, cout in ((buf_in[1:141], None), (flat, buf_out[1:141]), (buf_in[1:141], buf_out[3:143])):
        got = _run(cin, [9], K=0.01, sig_read=0.02, exposure=0.37, out=cout)
        assert torch.equal(got, want)
        if cout is not None:                                         # nothing written outside the view
            lo = (cout.data_ptr() - buf_out.data_ptr()) // 4
            assert (buf_out[:lo] == -7.0).all() and (buf_out[lo + 140:] == -7.0).all()
            buf_out.fill_(-7.0)


@pytest.mark.parametrize("layout", [CN.LAYOUT_PLANAR, CN.LAYOUT_BAYER])
def test_geometry_independence(layout):
    """Every term on, three items with their own parameters: together or one at a time, in place or not, aligned or not."""
    shape = (3, 4, 10, 28) if layout == CN.LAYOUT_PLANAR else (3, 20, 28)
    clean = _frames(shape, 3)
    slots = [7, 8, 9]
    both = _run(clean, slots, layout=layout, **ALL_ON)
    assert torch.isfinite(both).all()
    for b in range(3):
        one = {k: (v[b] if isinstance(v, list) else v) for k, v in ALL_ON.items()}
        assert torch.equal(_run(clean[b].clone(), [slots[b]], layout=layout, **one), both[b]), b
    assert not torch.equal(both[0], both[1])
    y = clean.clone()
    assert _run(y, slots, layout=layout, out=y, **ALL_ON) is y and torch.equal(y, both)
    n = clean[0].numel()
    buf = torch.zeros(n + 8, device=DEV)
    one = {k: (v[1] if isinstance(v, list) else v) for k, v in ALL_ON.items()}
    for off in (1, 2, 3):
        v = buf[off:off + n].view(shape[1:])
        v.copy_(clean[1])
        assert torch.equal(_run(v, [slots[1]], layout=layout, row_len=28, **one), both[1]), off
        _run(v, [slots[1]], layout=layout, row_len=28, out=v, **one)                    # in place, not aligned
        assert torch.equal(v, both[1]) and (buf[:off] == 0).all() and (buf[off + n:] == 0).all()
        buf.zero_()


def test_row_noise_only(golden):
    s, h, w = 0.05, 6, 8
    clean = torch.full((4, h, w), 0.25, device=DEV)
    d = (_run(clean, sig_row=s, K=0.0) - clean).cpu().numpy()
    assert np.array_equal(d, np.broadcast_to(d[:, :, :1], d.shape))                    # one value per row, exactly
    assert len(np.unique(d[:, :, 0])) == 4 * h                                         # rows of different planes are independent
    # the reference's structure (generate_noisy_obs, code r, on the same shape): constant along w, distinct along (c, h)
    g = golden("camnoise")
    ref = g["obs_r"].astype(np.float64) - g["obs_clean"]
    assert ref.shape == d.shape and ref.std(axis=2).max() < 1e-6 < 1e-4 < ref.mean(axis=2).std()
    assert len(np.unique(np.round(ref.mean(axis=2), 6))) == 4 * h
    # Bayer: one value per sensor row; the row draw is a function of (key, slot, row), so row r of either layout gets the same float
    db = (_run(clean.view(4 * h, w), layout=CN.LAYOUT_BAYER, sig_row=s) - clean.view(4 * h, w)).cpu().numpy()
    assert np.array_equal(db, d.reshape(4 * h, w))
    assert not np.array_equal((_run(clean, [1], sig_row=s) - clean).cpu().numpy(), d)
    # 2^14 rows of 4 (a float4 group per row) and of 6 (groups straddle rows)
    for w in (4, 6):
        c = torch.full((2 ** 14, w), 0.5, device=DEV)
        r = (_run(c, layout=CN.LAYOUT_BAYER, sig_row=s) - c).double().cpu().numpy()
        assert np.array_equal(r, np.broadcast_to(r[:, :1], r.shape))
        bad = CS.check_moments(r[:, 0], 0.0, float(np.float32(s)) ** 2, 3 * float(np.float32(s)) ** 4, f"row values, rows of {w}")
        assert not bad, bad
    # a plane boundary inside a float4 group: [4][3][2] has 6 elements per plane
    c = torch.zeros(4, 3, 2, device=DEV)
    r = _run(c, sig_row=s, bias=[1.0, 2.0, 3.0, 4.0]).cpu().numpy()
    rows = _run(torch.zeros(12, 2, device=DEV), layout=CN.LAYOUT_BAYER, sig_row=s).cpu().numpy().reshape(4, 3, 2)
    assert np.array_equal(r, rows + np.arange(1, 5, dtype=np.float32)[:, None, None])


def test_quantisation_only():
    n, q = 2 ** 20, 2.0 ** -10
    clean = _frames((n,), 4, 0.0, 1.0)
    noisy = _run(clean, q_step=q)
    ulp = torch.from_numpy(np.spacing(np.maximum(clean.cpu().numpy(), noisy.cpu().numpy()))).to(DEV)
    assert ((noisy - clean).abs() <= q / 2 + ulp).all()
    d = _run(torch.zeros(n, device=DEV), q_step=q).double().cpu().numpy()
    assert np.abs(d).max() < q / 2
    bad = CS.check_moments(d, 0.0, q * q / 12, q ** 4 / 80, "quantisation noise")
    assert not bad, bad
    # not divided by the root of MultiFrameMean
    assert np.array_equal(_run(torch.zeros(n, device=DEV), q_step=q, mfm=4).double().cpu().numpy(), d)


def test_bias_only():
    bias = np.array([1.0, -2.0, 3.0, 0.5], np.float32) / 8
    for layout, shape in ((CN.LAYOUT_PLANAR, (4, 5, 7)), (CN.LAYOUT_BAYER, (6, 10)), (CN.LAYOUT_BAYER, (5, 7))):
        clean = _frames(shape, 5, 0.0, 1.0)
        noisy = _run(clean, layout=layout, bias=bias).cpu().numpy()
        c = clean.cpu().numpy()
        if layout == CN.LAYOUT_PLANAR:
            ch = np.broadcast_to(np.arange(4)[:, None, None], shape)
        else:
            row, col = np.mgrid[0:shape[0], 0:shape[1]]
            ch = 2 * (row & 1) + (col & 1)
        want = c.astype(np.float64) + bias[ch]
        assert (np.abs(noisy - want) <= np.spacing(np.abs(want).astype(np.float32))).all(), (layout, shape)
        assert len(np.unique(np.round(noisy.astype(np.float64) - c, 5))) == 4
    # the mosaic's channel is bayer2rggb's plane
    x = torch.zeros(6, 10, device=DEV)
    planes = torch.empty(3, 5, 4, device=DEV)                       # [H / 2][W / 2][4]
    lib = _lib.load()
    noisy = _run(x, layout=CN.LAYOUT_BAYER, bias=bias)
    _lib.check(lib.yond_bayer2rggb_f32(_lib.ptr(noisy), 6, 10, _lib.ptr(planes), _lib.stream()), "yond_bayer2rggb_f32")
    assert np.array_equal(planes.cpu().numpy(), np.broadcast_to(bias, (3, 5, 4)))


def test_tukeylambda_read_noise():
    n, bad = 2 ** 20, []
    zeros = torch.zeros(n, device=DEV)
    for slot, lam in enumerate(CS.LAMS):
        t = _run(zeros, [slot], sig_read=1.0, lam=lam, tukey=True)
        row, fails = CS.check_tukeylambda(t.cpu().numpy(), float(np.float32(lam)))
        print(row + ("   FAIL: " + "; ".join(fails) if fails else ""))
        bad += [f"lam {lam}: {f}" for f in fails]
    assert not bad, bad
    # the scale is a scale, and the root of MultiFrameMean divides it
    t = _run(zeros, [4], sig_read=1.0, lam=0.102, tukey=True)
    assert torch.equal(_run(zeros, [4], sig_read=0.5, lam=0.102, tukey=True), t * 0.5)
    assert torch.equal(_run(zeros, [4], sig_read=1.0, lam=0.102, tukey=True, mfm=16), t * 0.25)
    # without the flag the read noise is Gaussian whatever lam says: the PG kernel's
    assert torch.equal(_run(zeros, [4], sig_read=1.0, lam=0.102), PG.add_pg_noise(zeros, 0.0, 1.0, 1.0, KEY, [4]))


def _sum_moments(parts):
    """(variance, fourth central moment) of a sum of independent zero-mean terms given as (variance, fourth moment) each."""
    var = sum(v for v, _ in parts)
    m4 = sum(m for _, m in parts) + 6 * sum(parts[i][0] * parts[j][0] for i in range(len(parts)) for j in range(i))
    return var, m4


@pytest.mark.parametrize("M", [1, 4])
def test_pg_total_variance(M):
    """Code pg (+ q with MultiFrameMean 4): constant clean at a shot lambda on either side of PG_SWITCH_PTRS, Tukey-lambda read noise
    lam = 0.102.  With m = sqrt(M) the reference divides the shot and read terms by m (k ~ Poisson(m lambda): variance lambda beta1^2 /
    m) and leaves the quantisation term alone."""
    assert PG.SWITCH_LAMBDAS[0] == 10.0
    n, s, lam_tl, m = 2 ** 20, 0.04, 0.102, math.sqrt(M)
    q = 2.0 ** -5 if M > 1 else 0.0
    var_tl, m4_tl = CN.tukeylambda_variance(lam_tl), CS.tl_moment4(lam_tl)
    for slot, lam in enumerate((9.0 / m, 12.0 / m)):                 # m * lambda = 9 and 12: inversion and PTRS
        clean = torch.full((n,), lam * BETA1, device=DEV)
        noisy = _run(clean, [slot], K=BETA1, sig_read=s, lam=lam_tl, tukey=True, q_step=q, mfm=M).double().cpu().numpy()
        L = m * lam
        parts = [(L * (BETA1 / m) ** 2, (L + 3 * L * L) * (BETA1 / m) ** 4), ((s / m) ** 2 * var_tl, (s / m) ** 4 * m4_tl),
                 (q * q / 12, q ** 4 / 80)]
        var, m4 = _sum_moments(parts)
        bad = CS.check_moments(noisy, lam * BETA1, var, m4, f"M {M}, shot lambda {L}: pg{'q' if q else ''} total")
        assert not bad, bad
        assert parts[0][0] > 0.1 * var and parts[1][0] > 0.1 * var   # both terms carry weight in the check


def test_mfm_divides_what_the_reference_divides():
    """Row and read terms by the root of MultiFrameMean, exactly (powers of two); the Gaussian shot approximation's moments."""
    s = 0.05
    c = torch.zeros(64, 8, device=DEV)
    r1 = _run(c, layout=CN.LAYOUT_BAYER, sig_row=s)
    r4 = _run(c, layout=CN.LAYOUT_BAYER, sig_row=s, mfm=4)
    assert torch.equal(r4, r1 / 2) and r1.abs().max() > 0
    g1 = _run(torch.zeros(4096, device=DEV), sig_read=s)
    assert torch.equal(_run(torch.zeros(4096, device=DEV), sig_read=s, mfm=16), g1 / 4)
    # shot noise without p: y + z sqrt(y / beta1) beta1 / m -- mean y, variance y beta1 / M
    n, y = 2 ** 20, 0.25
    for M in (1, 4):
        noisy = _run(torch.full((n,), y, device=DEV), K=BETA1, poisson=False, mfm=M).double().cpu().numpy()
        var = y * BETA1 / M
        bad = CS.check_moments(noisy, y, var, 3 * var * var, f"Gaussian shot approximation, M {M}")
        assert not bad, bad


def test_clip_stands_before_the_ratio():
    e, lo, hi = float(np.float32(0.01)), -0.0625, 1.0
    clean = _frames((4, 32, 48), 6, -10.0, 150.0)
    kw = dict(K=0.01, sig_read=0.02, lam=-0.026, tukey=True, sig_row=0.01, q_step=2.0 ** -10, bias=[0.01, 0.0, -0.01, 0.02], exposure=e)
    free = _run(clean, **kw)
    clipped = _run(clean, clip=(lo, hi), **kw)
    lo_e, hi_e = float(np.float32(lo) / np.float32(e)), float(np.float32(hi) / np.float32(e))
    assert free.min() < lo_e and free.max() > hi_e and abs(hi_e - 100) < 1e-3 and abs(lo_e + 6.25) < 1e-4
    assert clipped.min() == lo_e and clipped.max() == hi_e                             # [clip_lo / e, clip_hi / e], not [clip_lo, clip_hi]
    assert torch.equal(clipped, free.clamp(lo_e, hi_e))
    # the reference's sensor clip through the noise-code interface: [-bl / wp, 1] before the ratio
    p = dict(K=2.0, sigGs=8.0, sigTL=4.0, sigR=1.0, lam=-0.026, bias=[1, 2, 3, 4], wp=1023, bl=64)
    frame = _frames((64, 96), 7, -10.0, 150.0)
    out = CN.add_camera_noise(frame, p, "pgrqd", 959.0, KEY, [0], layout=CN.LAYOUT_BAYER, ratio=100, clip="sensor")
    assert out.min() == float(np.float32(-64 / 1023) / np.float32(0.01)) and out.max() == float(np.float32(1) / np.float32(0.01))


def test_edges():
    n = 2 ** 12
    x = _frames((4, 16, 64), 8, 0.0, 1.0)
    one = {k: (v[0] if isinstance(v, list) else v) for k, v in ALL_ON.items()}
    bad = {5: float("nan"), 64: float("inf"), 1001: float("-inf"), n - 1: float("nan")}
    xb = x.clone()
    for i, val in bad.items():
        xb.view(-1)[i] = val
    for kw in (one, dict(one, poisson=False), dict(one, tukey=False), dict(sig_row=0.1), dict(q_step=0.1), dict(bias=[1, 2, 3, 4]), dict()):
        yb = _run(xb, **kw).view(-1)
        nan = torch.isnan(yb).nonzero().flatten().tolist()
        assert nan == sorted(bad) and torch.isfinite(yb).sum().item() == n - len(bad), (kw, nan)
    # finite everywhere: huge x, denormal beta1 (lambda overflows), huge lambda, both shot models
    ext = torch.tensor([0.0, 1e-30, 1.0, 3e38, 1e30, 65504.0, -3e38, 0.5], device=DEV)
    for b1 in (BETA1, 1e-42, 1e-30, 1e30):
        for poisson in (True, False):
            ye = _run(ext, K=b1, sig_read=0.1, lam=-0.26, tukey=True, q_step=0.1, poisson=poisson)
            assert torch.isfinite(ye).all(), (b1, poisson, ye)
    # x < 0 carries through: the other terms are those of x = 0 at the same index
    s = 0.125
    neg = _run(torch.full((n,), -0.25, device=DEV), K=BETA1, sig_read=s)
    zero = _run(torch.zeros(n, device=DEV), K=BETA1, sig_read=s)
    assert torch.equal(neg, zero - 0.25)                            # s * z exact in both, -0.25 + s z: one rounding each
    neg = _run(torch.full((4, 16, 64), -0.25, device=DEV), **one)
    zero = _run(torch.zeros(4, 16, 64, device=DEV), **one)
    assert (neg - (zero - 0.25)).abs().max() <= 4 * 2.0 ** -24 * max(1.0, zero.abs().max().item())
    assert zero.std() > 0.01


def test_refusals_and_cpu_tensors():
    lib = _lib.load()
    clean = torch.zeros(4, 6, 8, device=DEV)
    out = torch.full_like(clean, -7.0)
    items = CN.plan(1, BETA1, 0.1, 1.0, KEY, [0], sig_row=0.1, bias=[1, 2, 3, 4])
    d_items = torch.from_numpy(items.view(np.uint8)).to(DEV)
    ok = dict(clean=_lib.ptr(clean), noisy=_lib.ptr(out), n=192, B=1, items=ctypes.c_void_p(d_items.data_ptr()), layout=0, row_len=8,
              stream=_lib.stream())

    def call(**kw):
        return lib.yond_camera_noise_f32(*dict(ok, **kw).values())
    for kw in (dict(clean=None), dict(noisy=None), dict(items=None), dict(B=0), dict(B=65536), dict(n=0),
               dict(clean=ctypes.c_void_p(clean.data_ptr() + 2)), dict(noisy=ctypes.c_void_p(out.data_ptr() + 1)),
               dict(layout=2), dict(layout=-1), dict(row_len=-8), dict(row_len=7), dict(row_len=5), dict(n=190, row_len=2),
               dict(layout=1, row_len=7), dict(layout=1, n=2 ** 32, row_len=8)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (out == -7.0).all()                                      # nothing was launched
    assert call() == 0 and call(layout=1) == 0 and call(row_len=48) == 0 and call(row_len=0) == 0
    torch.cuda.synchronize()
    assert (out != -7.0).all()
    # the Python launch knows the items: a geometry that does not divide them is refused when a term needs it, not otherwise
    with pytest.raises(ValueError, match="do not divide"):
        CN.launch(clean.view(-1)[:140], items)
    with pytest.raises(ValueError, match="do not divide"):
        CN.launch(clean, items, row_len=7)
    with pytest.raises(ValueError, match="do not divide"):
        CN.launch(clean.view(-1)[:190].view(19, 10), items)         # layout 0 needs four planes
    with pytest.raises(ValueError, match="layout"):
        CN.launch(clean, items, layout=2)
    with pytest.raises(ValueError, match="items of one size"):
        CN.launch(clean.view(-1)[:191], CN.plan(2, BETA1, 0.1, 1.0, KEY, [0, 1]))
    CN.launch(clean.view(-1)[:140], CN.plan(1, BETA1, 0.1, 1.0, KEY, [0], q_step=0.1, lam=0.1, tukey=True))
    with pytest.raises(Exception, match="ROCm device"):
        CN.add_camera_noise(torch.zeros(4, 6, 8), dict(K=1.0, sigGs=1.0), "p", 959.0, 0, [0])
    with pytest.raises(Exception, match="ROCm device"):
        CN.launch(clean, items, out=torch.zeros(4, 6, 8))


# -- --camera-noise in the full-frame driver -----------------------------------------------------------------------------------
def test_camera_noise_driver(tmp_path, monkeypatch):
    """`YOND_any --synthetic 2` on 512 x 768 frames at ratio 2: --camera-noise code=p,K=4,sigGs=6 is --synth-noise 4,6 -- the frames
    the two drivers make are equal bit for bit and so is the truth they report; what the estimator derives from a frame (reg, the
    relative errors, PSNR) is not bit-reproducible between two runs of ONE driver on ONE frame (float64 atomics in its moment sums:
    measured here, reg 0.008374410835856137 against 0.00837441083585613), so those are held to the bounds the project holds between
    two such runs (tests/test_hip_rawio.py, tests/test_hip_eval.py: round-1 estimates to rtol 1e-9, PSNR within 2e-3 dB).
    code=pgrqd reports the Poisson-Gaussian level of its variance as the truth, the estimator's relative error per round and the
    dark bias; both flags together exit."""
    import yaml
    from yond_public_amd import YOND_full as Y
    monkeypatch.chdir(tmp_path)
    H, W = 512, 768
    cfg = yaml.load(open(os.path.join(ROOT, "runfiles", "YOND", "ANY_simple+full_pre_grumix.yml")).read(), Loader=yaml.FullLoader)
    for sec in ('dst', 'dst_eval', 'dst_test'):
        cfg[sec].update(root_dir=str(tmp_path / "nowhere"), H=H, W=W, ratio_list=[2])
    rf = tmp_path / "any.yml"
    rf.write_text(yaml.dump(cfg))
    base = ['-f', str(rf), '-m', 'eval', '--synthetic', '2']
    with pytest.raises(SystemExit, match="exclude each other"):
        Y.YOND_Full(base + ['--synth-noise', '4,6', '--camera-noise', 'code=p,K=4,sigGs=6'])
    pg = Y.YOND_Full(base + ['--synth-noise', '4,6'])
    res_pg = pg.eval(-1)
    cam = Y.YOND_Full(base + ['--camera-noise', 'code=p,K=4,sigGs=6'])
    assert type(cam.dst_eval).__name__ == 'SyntheticFrames' and cam.dst_eval.clean_only and cam.synth_noise is None
    res_cam = cam.eval(-1)
    assert len(cam.metrics) == 2 and sorted(cam.metrics) == sorted(pg.metrics) and sorted(res_cam) == sorted(res_pg) == ['x2']
    wp, bl = float(cam.dst.get('wp', 1023)), float(cam.dst.get('bl', 64))
    for k in range(2):
        item = cam.dst_eval[k]
        a, b = cam.synthesise(dict(item), wp, bl), pg.synthesise(dict(pg.dst_eval[k]), wp, bl)
        assert torch.equal(a['lr'], b['lr']) and torch.equal(a['hr'], b['hr']) and not torch.equal(a['lr'], a['hr'])
        mc, mp = cam.metrics[item['name']], pg.metrics[item['name']]
        assert sorted(mc) == sorted(mp) == ['psnr', 'reg', 'rel_err', 'ssim', 'true']
        assert mc['true'] == mp['true'] == (8.0, 12.0)
        assert len(mc['reg']) == len(mp['reg']) and len(mc['psnr']) == len(mp['psnr']) and len(mc['rel_err']) == len(mp['rel_err'])
        np.testing.assert_allclose(np.asarray(mc['reg'][0], np.float64), np.asarray(mp['reg'][0], np.float64), rtol=1e-9)
        np.testing.assert_allclose(np.asarray(mc['rel_err'][0], np.float64), np.asarray(mp['rel_err'][0], np.float64), rtol=0,
                                   atol=2e-9)                     # |q - K| / K with q to rtol 1e-9 and q < 2 K
        assert all(abs(x - y) < 2e-3 for x, y in zip(mc['psnr'], mp['psnr']))
    assert res_cam['x2']['count'] == res_pg['x2']['count'] == 2
    assert abs(res_cam['x2']['rel_err_K_iter0'] - res_pg['x2']['rel_err_K_iter0']) <= 2e-9

    spec = 'code=pgrqd,K=4,sigTL=3,sigGs=6,sigR=2,lam=-0.026,bias=1/-2/3/0.5'
    full = Y.YOND_Full(base + ['--camera-noise', spec])
    res = full.eval(-1)
    K, sig = CN.effective_pg(dict(K=4.0, sigTL=3.0, sigR=2.0, lam=-0.026), 'pgrqd')
    assert K == 4.0 and sig == pytest.approx(math.sqrt(9 * CN.tukeylambda_variance(-0.026) + 4 + 1 / 12), rel=1e-15)
    assert set(res) == {'x2'} and res['x2']['count'] == 2 and np.isfinite(res['x2']['rel_err_K_iter0'])
    assert np.isfinite(res['x2']['rel_err_sigma_iter0'])
    for name, m in full.metrics.items():
        assert m['true'] == (2 * K, 2 * sig) and m['bias'] == [2.0, -4.0, 6.0, 1.0]
        assert 1 <= len(m['rel_err']) <= 2 and all(len(e) == 2 and np.isfinite(e).all() for e in m['rel_err'])
        assert m['psnr'] != pg.metrics[name]['psnr']
        print(f"{name}: rounds {m['psnr']}, rel err (K, sigma) per round {m['rel_err']}")
    log = open(tmp_path / "logs" / f"log_{cfg['method_name']}.log").read()
    assert f"true K={2 * K:.3f}, sigma={2 * sig:.3f}, dark bias 2.000/-4.000/6.000/1.000" in log
    assert "mean |K_est - K| / K" in log and "mean |sigma_est - sigma| / sigma" in log
