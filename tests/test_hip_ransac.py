"""GPU: the robust noise-level fit -- utils.polyfit(x, y, ransac=True) (ransac.hip) against the reference's own results
(tests/golden/ransac.npz) and the float64 model (tests/ransac_model.py); the compaction order of SimpleNLF(fit='ransac'); determinism;
IterDenoise with est_fit 'ransac'."""
import numpy as np
import pytest
import torch

import ransac_model as RM
from hip_common import ARCHS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope="module")
def fits():
    return {name: RM.fit(*RM.make_points(name)) for name in RM.CASES}


@pytest.mark.parametrize("name", list(RM.CASES))
def test_polyfit_ransac_matches_reference(golden, fits, name):
    """The function path on every golden case: one workgroup (n = 300), n = 4096, ragged tiles over several workgroups (n = 5000:
    five compaction tiles, three scoring chunks), the early stop (8 of 100 trials), both sides of the 1 % non-saturation rule.
    Bounds: the threshold bit for bit (float32 order statistics and one float32 mean); the trials' lines to 1e-9 of their scale -- the
    kernel's centred float64 sums and the model's SVD of [x, 1] both carry ~cond^2 eps <= ~1e-12 here (cond <= ~20 for these x
    ranges), so 1e-9 is three orders above either and seven below a wrong subset; the counts exact outside the model's 1e-6 band
    around the threshold; (beta1, beta2) to the fit bound of DESIGN section 1 rows D / E against the reference's result.
    MEASURED (MI355X): see DESIGN section 3."""
    from yond_public_amd import utils as U
    g, r = golden("ransac"), fits[name]
    x, y = RM.make_points(name)
    reg, info = U.polyfit(x, y, ransac=True, _full=True)
    ref = g[f"{name}_res"]
    tab = info['table']                               # the rows computed: whole batches of (2, 4, 8, ...) trials until sklearn's loop ends
    R = len(tab)
    assert info['n_trials'] <= R <= RM.TRIALS and (R == RM.TRIALS or R in (2, 6, 14, 30, 62))
    lines = r["lines"][:R]
    scale_b = np.abs(lines[:, 1]) + np.abs(lines[:, 0]) * float(np.abs(r["x"]).max())
    da = np.abs(tab[:, 0] - lines[:, 0]) / np.abs(lines[:, 0])
    db = np.abs(tab[:, 1] - lines[:, 1]) / scale_b
    dcount = np.abs(tab[:, 2].astype(np.int64) - r["counts"][:R])
    print(f"[ransac] {name}: rows={R} n={info['n']} m={info['m']} thr={info['thr']!r} winner={info['winner']} inliers={info['n_inliers']} "
          f"trials={info['n_trials']}; lines max rel slope {da.max():.2e}, intercept {db.max():.2e} of scale; counts max diff {dcount.max()}; "
          f"|d beta1|/beta1 = {abs(reg[0] - ref[0]) / abs(ref[0]):.2e}, |d beta2| = {abs(reg[1] - ref[1]):.2e} "
          f"(bound {1e-5 * abs(ref[0]) + 1e-9:.2e})")
    assert (info['n'], info['m']) == (int(g[f"{name}_n"]), int(g[f"{name}_m"])) and info['nonsat'] == r["masked"]
    assert np.float32(info['thr']) == g[f"{name}_thr"] == RM.mad_threshold(r["y"])                   # bit-equal to NumPy's float32 value
    assert np.all(tab[:, 9] == np.float64(g[f"{name}_thr"]))
    assert da.max() <= 1e-9 and db.max() <= 1e-9
    assert np.all(dcount <= r["near"][:R])
    if int(g[f"{name}_n_trials"]) == RM.TRIALS:
        assert R == RM.TRIALS                         # (five of the seven cases: all 100 lines and counts are compared)
    if RM.CASES[name]["winner"]:
        assert info['winner'] == r["winner"]
    assert info['n_inliers'] == int(g[f"{name}_n_inliers"]) and info['n_trials'] == int(g[f"{name}_n_trials"])
    assert abs(reg[0] - ref[0]) <= 1e-5 * abs(ref[0]) and abs(reg[1] - ref[1]) <= 1e-5 * abs(ref[0]) + 1e-9
    # the inlier sums of the winner against float64 NumPy sums over the same inliers (pairwise there, tree order here: ~n eps)
    a, b = tab[info['winner'], :2]
    xd, yd = r["x"].astype(np.float64), r["y"].astype(np.float64)
    res = np.abs(yd - (a * xd + b))
    i = res <= np.float64(info['thr'])
    want = np.array([xd[i].sum(), yd[i].sum(), (xd[i] ** 2).sum(), (xd[i] * yd[i]).sum(), (yd[i] ** 2).sum(), (res[i] ** 2).sum()])
    if int(i.sum()) == info['n_inliers']:
        np.testing.assert_allclose(tab[info["winner"], 3:9], want, rtol=2e-12)      # 2 n eps, n <= 5000: both summations at their worst


def test_polyfit_ransac_device_tensors_and_errors():
    from yond_public_amd import utils as U
    from yond_public_amd._lib import YondHipError
    x, y = RM.make_points("n300_c30")
    a = U.polyfit(x, y, ransac=True)
    b = U.polyfit(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), ransac=True)
    assert len(a) == 2 and tuple(a) == tuple(b)
    with pytest.raises(YondHipError):
        U.polyfit(x[:1], y[:1], ransac=True)
    lsq = U.polyfit(x, y)                                          # the default branch is untouched and differs on contaminated points
    assert tuple(lsq) != tuple(a)


def test_ransac_is_deterministic():
    """Two runs: (beta1, beta2) and the whole trial table -- counts and every float64 sum -- bit for bit (no float64 atomics)."""
    from yond_public_amd import utils as U
    x, y = RM.make_points("n5000_c20")
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    r1, i1 = U.polyfit(xd, yd, ransac=True, _full=True)
    r2, i2 = U.polyfit(xd, yd, ransac=True, _full=True)
    assert np.array_equal(np.asarray(r1).view(np.uint64), np.asarray(r2).view(np.uint64))
    assert np.array_equal(i1['table'].view(np.uint64), i2['table'].view(np.uint64))
    assert np.array_equal(i1['table'][:, 2], i2['table'][:, 2]) and i1['table'][:, 2].max() > 0


def _textured_frame(H, W, seed, amp=0.12):
    """A Poisson-Gaussian frame (K = 4, sigma = 6 DN on a 959 DN scale) of a smooth scene whose top-left quarter carries a texture of
    amplitude `amp` (the noise deviation is ~0.04 at mid-grey)."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    clean = 0.15 + 0.5 * xx / W + 0.1 * yy / H
    tex = amp * np.sign(np.sin(xx * 1.3) * np.sin(yy * 0.9))
    clean[:H // 2, :W // 2] += tex[:H // 2, :W // 2]
    clean = np.clip(clean, 0.02, 0.95)
    scale, K, sig = 959.0, 4.0, 6.0
    noisy = (rs.poisson(clean * scale / K) * K + rs.normal(0.0, sig, clean.shape)) / scale
    return noisy.astype(np.float32)


@pytest.mark.parametrize("mode,H,W,sidd", [("self", 64, 96, False), ("collab", 64, 96, False), ("collab", 64, 512, True), ("self", 64, 512, True)])
def test_simple_nlf_ransac_compaction_order(mode, H, W, sidd):
    """SimpleNLF(fit='ransac') on a Bayer frame with k = 5 equals utils.polyfit(mean[mask], var[mask], ransac=True) fed host arrays
    gathered from the same device maps in the reference's indexing ([h][w][4]; with SIDD_256 the [h][w / 32][128] of
    YOND_SIDD.py:65, 92-93): the subsets index the points by position, so any other order gives other trials.  The same points in
    the same order give the same bits."""
    from yond_public_amd import pipeline as P
    from yond_public_amd import utils as U
    lr = torch.from_numpy(_textured_frame(H, W, 5)).to(DEV)
    hr = None
    if mode == "collab":
        sm = torch.nn.functional.avg_pool2d(lr[None, None], 3, 1, 1, count_include_pad=False)[0, 0]
        hr = (0.5 * lr + 0.5 * sm).contiguous()
    setting = {'mode': mode, 'SIDD_256': sidd}
    reg, info = P.SimpleNLF(lr, hr, k=5, setting=dict(setting, fit='ransac'), full=True)
    lsq = P.SimpleNLF(lr, hr, k=5, setting=setting)
    lap, mean, var, _ = P.SimpleNLF(lr, hr, k=5, setting=setting, _maps_only=True)
    hwc = lambda t: t.permute(1, 2, 0).cpu().numpy()
    lap, mean, var = hwc(lap), hwc(mean), hwc(var)
    if sidd:
        lap, mean, var = (np.concatenate(np.split(a, 32, axis=-2), axis=-1) for a in (lap, mean, var))
        assert lap.shape == (H // 2, W // 64, 128)
    mask = lap.astype(np.float64) < np.float64(info['th'])
    assert 100 < mask.sum() < mask.size
    want, winfo = U.polyfit(mean[mask], var[mask], ransac=True, _full=True)
    ri = info['ransac']
    print(f"[ransac] {mode} sidd={sidd}: selected {ri['n_selected']}, fitted {ri['n']}, winner {ri['winner']} with {ri['n_inliers']} inliers, "
          f"{ri['n_trials']} trials; ransac {tuple(reg)} lsq {tuple(lsq)}")
    assert ri['n_selected'] == int(mask.sum()) and ri['n'] == winfo['n']
    assert (ri['winner'], ri['n_inliers'], ri['n_trials']) == (winfo['winner'], winfo['n_inliers'], winfo['n_trials'])
    assert np.array_equal(ri['table'][:, 2], winfo['table'][:, 2])
    assert np.array_equal(ri['table'].view(np.uint64), winfo['table'].view(np.uint64)) and tuple(reg) == tuple(want)
    # a shuffled order is a different problem (the check above can tell orders apart)
    perm = np.random.RandomState(0).permutation(int(mask.sum()))
    _, sinfo = U.polyfit(mean[mask][perm], var[mask][perm], ransac=True, _full=True)
    assert not np.array_equal(sinfo['table'][:, 2], ri['table'][:, 2])


def test_iter_denoise_est_fit():
    """IterDenoise with est_fit 'ransac' on a 64 x 64 frame with a textured quarter and a tiny net: off the device chain, round 1's
    estimate is SimpleNLF(fit='ransac')'s, the result differs from the least-squares run's, and 'lsq' is the run without the key."""
    from yond_public_amd import archs as A
    from yond_public_amd import pipeline as P
    from yond_public_amd import synthetic as S
    arch = ARCHS["gru8"]
    net = A.GuidedResUnet(dict(arch))
    net.load_state_dict(S.denoising_state_dict(net, 3))
    net = net.to(DEV).eval()
    # (texture at the noise's own level: the least-squares line is bent, (0.0012, 0.0020) against RANSAC's (0.0022, 0.0013) in the
    # float64 model, and both stay positive so that both runs denoise)
    x = torch.from_numpy(_textured_frame(64, 64, 9, amp=0.04)).to(DEV)
    pipe = {'k': 5, 'vst_type': 'exact', 'bias_corr': 'pre', 'iter': 'iter', 'max_iter': 1, 'full_dn': True}
    assert P.chain_applies(x, net, arch, pipe) and P.chain_applies(x, net, arch, dict(pipe, est_fit='lsq'))
    assert not P.chain_applies(x, net, arch, dict(pipe, est_fit='ransac'))
    base = P.IterDenoise(x, net, arch, pipe)
    lsq = P.IterDenoise(x, net, arch, dict(pipe, est_fit='lsq'))
    rns = P.IterDenoise(x, net, arch, dict(pipe, est_fit='ransac'))
    assert len(base['raw_dns']) == len(lsq['raw_dns']) and len(rns['raw_dns']) >= 1
    for a, b in zip(base['raw_dns'], lsq['raw_dns']):
        assert torch.equal(a, b)
    assert [tuple(np.asarray(r, np.float64)) for r in base['regs']] == [tuple(np.asarray(r, np.float64)) for r in lsq['regs']]
    want = P.SimpleNLF(x, k=5, setting={'mode': 'self', 'fit': 'ransac'})
    assert tuple(rns['regs'][0]) == tuple(want)
    assert tuple(rns['regs'][0]) != tuple(np.asarray(lsq['regs'][0], np.float64))
    assert not torch.equal(rns['raw_dns'][0], lsq['raw_dns'][0])
    if len(rns['raw_dns']) > 1:                                    # round 2's collaborative estimate took the same fit
        can_tile = (x.shape[-1] // 2) % 32 == 0
        want2 = P.SimpleNLF(x, rns['raw_dns'][0], k=5, setting={'mode': 'collab', 'fit': 'ransac', 'SIDD_256': can_tile})
        got2 = rns['regs'][1]
        assert got2[0] == want2[0] and (got2[1] == want2[1] or (want2[1] < 0 and got2[1] == want2[0] ** 2))
    # the stream driver falls back to the same path, frame by frame
    st = list(P.denoise_stream([x, x], net, arch, dict(pipe, est_fit='ransac')))
    assert len(st) == 2 and all(torch.equal(s['raw_dns'][0], rns['raw_dns'][0]) for s in st)
    with pytest.raises(P.L.YondHipError):
        P.IterDenoise(x, net, arch, dict(pipe, est_fit='huber'))
