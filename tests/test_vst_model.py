"""CPU: the float64 models of tests/vst_model.py reproduce the oracle, the two-answer share of the edge cases keeps the ulp bound a
bit-exactness test, and single defects a correct kernel does not have exceed the bound (tests/test_hip_vst_edges.py holds the HIP
kernels to the same models and the same bound)."""
import functools

import numpy as np
import pytest

import vst_model as M


@functools.lru_cache(maxsize=None)
def _oracle_lut(mx, K, s):
    """get_bias' knots and float32 ordinates for a float32 frame maximum from the oracle (the GPU tests read the device-built ones back)."""
    import yond_oracle as O
    lams, bias = O.get_bias_table(np.float32(mx), np.float64(s), np.float64(K))
    return np.asarray(lams), np.asarray(bias, np.float32)


def _golden_biaslut():
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "biaslut.npz"))
    return g["table"], g["x_lut"], g["sg_lut"]


def case_lut(case):
    """(lut_x float64, lut_y, biaslut) of a K1 case on the CPU; the frame's maximum is known before the knot hits go in."""
    name, H, W, pads, K, s, bc, top, seed = case
    if bc is False:
        return None, None, False
    if bc == '2d':
        lx, ly = M.merged_row(*_golden_biaslut(), K, s)
        return lx, ly, True
    mx = M.frame_max_dn(M.k1_frame_base(H, W, K, s, top, seed))
    ub = np.ceil(mx) + 1                                                                   # float32, as the pipeline forms it
    if bc == 'synthetic':
        lx = np.asarray(M.bias_knots(ub), np.float64)
        return lx, M.synthetic_ordinates(lx), False
    lams, bias = _oracle_lut(float(mx), K, s)
    assert len(lams) == len(M.bias_knots(ub))
    return np.asarray(lams, np.float64), bias, False


def k1_case_ref(case, defect=None):
    name, H, W, pads, K, s, bc, top, seed = case
    lx, ly, two_d = case_lut(case)
    f = M.k1_frame(H, W, K, s, top, seed, None if two_d else lx)
    assert lx is None or two_d or M.frame_max_dn(f) <= lx[-1]
    lo, hi = M.lo_hi(K, s)
    return M.k1_ref(f, pads, 1, M.SCALE, K, s, lo, hi, lx, ly, two_d, defect=defect), (lo, hi)


def k4_case_ref(case, defect=None):
    name, (gname, Hp, Wp, pt, pl, h, w), mode, clip, K, s, lo, hi, zmin, seed = case
    y = M.k4_case_input(case)
    return M.k4_ref(y, pt, pl, h, w, mode, M.SCALE, K, s, lo, hi, clip, defect=defect)


# ---------------------------------------------------------------------------------------------------------------------------
# the models reproduce the oracle on the inputs of the existing K1 / K4 / metrics tests, at those tests' tolerances
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,K,s,bc", [(128, 192, 4.37, 6.27, True), (120, 136, 22.65, 37.09, True), (64, 96, 0.72, 1.8, True),
                                        (128, 128, 4.37, 6.27, False)])
def test_k1_model_reproduces_the_oracle(H, W, K, s, bc):
    import torch
    import torch.nn.functional as F
    import yond_oracle as O
    noisy, _ = O.synth_noisy(H, W, K, s, 3)
    K, s = np.float64(K), np.float64(s)
    lr = O.bayer2rggb(noisy) * 959.0
    v = O.VST(lr, s, gain=K)
    f = None
    if bc:
        f = O.get_bias(lr.max(), s, K)
        v = v - f(np.maximum(lr, 0))
    lo, hi = O.VST(0, s, gain=K), O.VST(959.0, s, gain=K)
    u = torch.from_numpy(np.ascontiguousarray((v - lo) / (hi - lo))).permute(2, 0, 1)[None]
    p2d = O.get_p2d(u.shape, 32)
    ref = F.pad(u, p2d, mode='reflect').clamp(0, 1)[0].permute(1, 2, 0).numpy()
    got, band = M.k1_ref(noisy, p2d, 1, 959.0, K, s, lo, hi, None if f is None else np.asarray(f.x, np.float64), None if f is None else f.y)
    assert got.dtype == np.float64 and np.abs(got - ref).max() <= 3e-7
    assert np.abs(got - ref).max() <= 1e-12                       # (in fact the same float64 staging)
    assert (lo, hi) == M.lo_hi(K, s)
    if f is not None:                                            # interp1d's own restatement, and np.interp but for the float32 difference
        xq = np.maximum(lr, 0).astype(np.float64)
        mine = M.lut1d(np.asarray(f.x, np.float64), f.y, xq)
        assert np.array_equal(mine, f(xq))
        assert np.abs(mine - np.interp(xq, np.asarray(f.x, np.float64), f.y.astype(np.float64))).max() <= 1e-7


def test_k1_model_2d_lut_reproduces_the_oracle():
    import yond_oracle as O
    table, x_lut, sg_lut = _golden_biaslut()
    lut = O.BiasLUT(table, x_lut, sg_lut)
    rng = np.random.default_rng(3)
    for (K, s) in ((0.72, 1.8), (0.05, 0.3), (4.37, 6.27), (120.0, 0.0)):
        lx, ly = M.merged_row(table, x_lut, sg_lut, K, s)
        xq = np.concatenate((rng.uniform(0, 1300, 4000), lx[lx <= 1300], [0.0])).astype(np.float32)
        want = lut.get_lut(xq.copy(), K=np.float64(K), sigGs=np.float64(s))
        got = M.lut2d(lx, ly, xq, K, s)
        x_pos = lut.pos_interp(lut.x_lut, xq / np.float64(K))
        print(f"[model] 2-D LUT K={K}: {(x_pos >= len(x_lut)).sum()} closed-form queries, {((x_pos > len(x_lut) - 1) & (x_pos < len(x_lut))).sum()} on the last ordinate")
        assert np.abs(got - want).max() <= 1e-10                  # the tolerance of test_bias_lut_2d_matches_reference in the table
    assert M.merged_row(table, x_lut, sg_lut, 1.0, 400.0) is None


def test_k4_model_reproduces_the_oracle():
    import yond_oracle as O
    rng = np.random.default_rng(5)
    Hp, Wp, h, w, pt, pl = 64, 96, 60, 90, 2, 3
    y = (rng.random((Hp, Wp, 4)) * 1.2 - 0.1).astype(np.float32)
    K, s = np.float64(4.37), np.float64(6.27)
    lo, hi = O.VST(0, s, gain=K), O.VST(959.0, s, gain=K)
    for mode, exact in ((1, False), (2, True)):
        yc = np.clip(y, 0, 1)[pt:pt + h, pl:pl + w]
        ref = O.rggb2bayer(O.inverse_VST(yc * (hi - lo) + lo, s, gain=K, exact=exact)) / 959.0
        got, band = M.k4_ref(y, pt, pl, h, w, mode, 959.0, K, s, lo, hi, 0)
        rel = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-6)
        assert rel.max() <= 2 ** -23
        assert rel.max() <= 1e-15 and np.all(np.abs(got - ref) <= band + 1e-300)
    # z <= 0 maps to 0 as the reference's masked assignment does (utils/isp_algos.py:21-25)
    z = np.array([-3.0, 0.0, 1e-3, 0.7, 2.0])
    ynet = np.tile(((z + 50.0) / 100.0).astype(np.float32)[:, None, None], (1, 1, 4))
    got, _ = M.k4_ref(ynet, 0, 0, 5, 1, 2, 959.0, K, s, -50.0, 50.0, 0)
    zz = np.clip(ynet, 0, 1).astype(np.float64) * 100.0 - 50.0
    np.testing.assert_allclose(got, O.rggb2bayer(O.inverse_VST(zz, s, gain=K, exact=True)) / 959.0, rtol=1e-15, atol=0)
    assert np.all(got[:4] == 0.0)


def test_metric_models_reproduce_the_oracle():
    import yond_oracle as O
    noisy, clean = O.synth_noisy(256, 1024, 4.0, 6.0, 41)
    dn = np.clip(clean + 0.01 * (noisy - clean), 0, 1).astype(np.float32)
    for a, b in zip(np.split(dn, 4, axis=-1), np.split(clean, 4, axis=-1)):
        assert abs(M.psnr_ref(a, b) - O.psnr(a, b)) <= 1e-6
        assert abs(M.ssim_ref(a, b) - O.ssim(a * 255, b * 255)) <= 1e-9
    rng = np.random.default_rng(1)
    a, b = rng.random((12, 43)).astype(np.float32), rng.random((12, 43)).astype(np.float32)
    assert abs(M.ssim_ref(a, b) - O.ssim(a * 255, b * 255)) <= 1e-12 and abs(M.ssim_ref(1 - a, a)) < 1 and M.ssim_ref(1 - a, a) < 0
    assert M.ssim_ref(a, a) == 1.0 and M.psnr_ref(a, a) == float('inf')
    assert np.array_equal(M.gauss11(), O._gauss_kernel())


# ---------------------------------------------------------------------------------------------------------------------------
# the bound itself
# ---------------------------------------------------------------------------------------------------------------------------
def test_ulp_check_admits_one_answer_outside_the_band_and_two_inside():
    v = np.array([0.75 + 2.0 ** -25 * 0.999, 0.75 + 2.0 ** -25 * (1 - 1e-6), 1.0, 0.0, 2.0 ** -149 * 0.3, 1e-40])
    near = v.astype(np.float32)
    up = np.nextafter(near, np.float32(2))
    band = np.full(v.shape, 1e-12)
    band[3] = 0.0
    assert M.ulp_check(near, v, band) == pytest.approx(3 / 6)     # the second, fifth and sixth: v within 1e-12 of a midpoint
    for i, ok in enumerate((False, True, False, False, True, True)):
        g = near.copy()
        g[i] = up[i]
        if ok:
            M.ulp_check(g, v, band)
        else:
            with pytest.raises(AssertionError):
                M.ulp_check(g, v, band)
    with pytest.raises(AssertionError):
        M.ulp_check(np.array([np.nan], np.float32), np.array([0.5]), 1e-12)
    assert M.ulp32(np.array([1.0, 0.99999, 0.0, 2.0 ** -126, 2.0 ** -127]))[[0, 1]].tolist() == [2.0 ** -23, 2.0 ** -24]
    assert M.ulp32(np.array([0.0, 2.0 ** -126, 2.0 ** -127])).tolist() == [2.0 ** -149] * 3


def test_two_answer_share_of_every_well_conditioned_case():
    """At most 1 % of a well-conditioned case's elements may admit two answers: the test stays a bit-exactness test.  From the
    reference alone (the knots are the oracle's); the ill-conditioned pair's share is only reported."""
    worst = 0.0
    for case in M.k1_cases():
        (u, band), (lo, hi) = k1_case_ref(case)
        share = float(M.two_answers(u, band).mean())
        wc = M.well_conditioned(lo, hi)
        print(f"[model] K1 {case[0]}: two-answer share {share:.2e} ({'well' if wc else 'ill'}-conditioned), {u.size} elements, "
              f"{int((u == 0).sum())} at 0, {int((u == 1).sum())} at 1")
        if wc:
            worst = max(worst, share)
            assert share <= M.SHARE_MAX, case[0]
    for case in M.k4_cases():
        r, band = k4_case_ref(case)
        share = float(M.two_answers(r, band).mean())
        wc = case[2] == 0 or M.well_conditioned(case[6], case[7])
        print(f"[model] K4 {case[0]}: two-answer share {share:.2e} ({'well' if wc else 'ill'}-conditioned)")
        if wc:
            worst = max(worst, share)
            assert share <= M.SHARE_MAX, case[0]
    print(f"[model] worst well-conditioned share {worst:.2e}")


def test_case_list_reaches_the_edges_it_names():
    """The statistics the cases are there for are really in them (a generator that silently drops them would leave the tests green)."""
    cases = {c[0]: c for c in M.k1_cases()}
    c = cases["main K=4.37 s=6.27 bc=1 top=1.0"]
    lx, ly, _ = case_lut(c)
    f = M.k1_frame(*c[1:3], *c[4:6], *c[7:9], lx)
    x32 = (f * np.float32(959.0)).astype(np.float64)
    assert (np.diff(lx) == 0).sum() == 2 and lx.dtype == np.float64
    for t in (50.0, 500.0, 51.0):                                 # (0.1 is not a float32 value: no pixel lands on it)
        t32 = np.float32(t)
        above = x32[(x32 > np.float64(t32)) & (x32 <= np.float64(t32) * (1 + 3 * 2.0 ** -23))]
        below = x32[(x32 < np.float64(t32)) & (x32 >= np.float64(t32) * (1 - 3 * 2.0 ** -23))]
        assert (x32 == np.float64(t32)).any() and above.size and below.size, t
    fz = 4.37 * x32 + 0.375 * 4.37 ** 2 + 6.27 ** 2
    assert (fz < 0).any() and ((x32 < 0) & (fz > 0)).any() and (f == 0).any() and ((f > 0) & (f < 1.1754944e-38)).any()
    runs = [int((np.diff(case_lut(cases[f"main K=4.37 s=6.27 bc=1 top={t}"])[0]) == 0).sum()) + 1 for t in M.K1_TOPS]
    assert runs == [1, 2, 3]
    assert M.bias_knots(np.float32(40.0)).dtype == np.float32 and M.bias_knots(np.float64(40.0)).dtype == np.float64
    (u, _), _ = k1_case_ref(cases["above white K=4.37 s=6.27"])
    assert (u == 1).sum() > u.size // 10
    for (name, H, W, pads) in M.K1_GEOMS:
        assert pads[0] <= W // 2 - 1 and pads[1] <= W // 2 - 1 and pads[2] <= H // 2 - 1 and pads[3] <= H // 2 - 1
    assert sorted(W // 2 + p[0] + p[1] for (_, H, W, p) in M.K1_GEOMS)[-7:] == [255, 256, 257, 511, 512, 513, 769]
    assert all(B * (H // 2 + p[2] + p[3]) > 1536 for (B, H, W, p) in M.K1_BATCH)
    assert [M.batch_crossings(B, H // 2 + p[2] + p[3]) > 0 for (B, H, W, p) in M.K1_BATCH] == [False, True, True]
    k4 = {c[0]: c for c in M.k4_cases()}
    name, g, mode, clip, K, s, lo, hi, zmin, seed = k4["z 1e-3..50 K=4.37 s=6.27"]
    c = k4["z 1e-3..50 K=4.37 s=6.27"]
    y = M.k4_case_input(c)[g[3]:g[3] + g[5], g[4]:g[4] + g[6]]
    z = np.clip(y, 0, 1).astype(np.float64) * (hi - lo) + lo
    r, band = M.k4_ref(M.k4_case_input(c), g[3], g[4], g[5], g[6], 2, 959.0, K, s, lo, hi, 0)
    assert z.min() < 2e-3 and z.max() > 45 and (r == 0).any() and ((r > 0) & (r < 1e-7)).any()      # either side of the zero crossing
    c = k4["z -50..50 K=4.37 s=6.27"]
    name, g, mode, clip, K, s, lo, hi, zmin, seed = c
    y = M.k4_case_input(c)[g[3]:g[3] + g[5], g[4]:g[4] + g[6]]
    z = np.clip(y, 0, 1).astype(np.float64) * (hi - lo) + lo
    assert (z < 0).any() and (z == 0).any() and g[3] + g[5] == g[1] and g[4] + g[6] == g[2]
    assert M.K4_BATCH[0] * M.K4_BATCH[5] > 4096


# ---------------------------------------------------------------------------------------------------------------------------
# single defects exceed the bound
# ---------------------------------------------------------------------------------------------------------------------------
# defects whose effect does not depend on the LUT's curvature must also show on the ill-conditioned pair (K, sigma) = (1, 400); the
# interval defects show there on the synthetic ordinates (get_bias' own ordinates are flat to 1e-9 / DN at sigma / K = 400)
@pytest.mark.parametrize("defect", M.K1_DEFECTS)
def test_k1_defect_exceeds_the_bound(defect):
    caught, caught_ill = [], []
    for case in M.k1_cases():
        if case[6] is False and defect in ('searchsorted_right', 'interval_off_by_one', 'lut_at_x'):
            continue
        (u, band), (lo, hi) = k1_case_ref(case)
        (ud, _), _ = k1_case_ref(case, defect)
        with np.errstate(invalid='ignore'):
            got = np.clip(ud, 0, 1).astype(np.float32)
        r = M.ulp_ratio(got, u, band)
        if r.max() > 1.0:
            (caught if M.well_conditioned(lo, hi) else caught_ill).append((case[0], float(min(r.max(), 1e300)), int((r > 1).sum())))
    for name, worst, nbad in (caught + caught_ill)[:6]:
        print(f"[model] K1 defect {defect}: fails {name}: worst ratio {worst:.3g}, {nbad} elements")
    print(f"[model] K1 defect {defect}: {len(caught)} well-conditioned and {len(caught_ill)} ill-conditioned cases fail")
    assert caught, defect
    assert caught_ill, defect


@pytest.mark.parametrize("defect", M.K4_DEFECTS)
def test_k4_defect_exceeds_the_bound(defect):
    caught = []
    for case in M.k4_cases():
        r, band = k4_case_ref(case)
        rd, _ = k4_case_ref(case, defect)
        ratio = M.ulp_ratio(rd.astype(np.float32), r, band)
        if ratio.max() > 1.0:
            caught.append(case[0])
    print(f"[model] K4 defect {defect}: fails {caught}")
    assert any(c.startswith("z -50..50") for c in caught)


@pytest.mark.parametrize("defect", M.N1_DEFECTS)
def test_n1_defect_exceeds_the_metric_tolerance(defect):
    caught = []
    for (gname, H, W, bh, bw) in M.N1_GEOMS:
        for kind in M.N1_PAIRS:
            dn, hr = M.n1_pair(kind, H, W, bh, bw)
            for a, b in zip(M.blocks(dn, bh, bw), M.blocks(hr, bh, bw)):
                ds = abs(M.ssim_ref(a, b, defect) - M.ssim_ref(a, b))
                p0, p1 = M.psnr_ref(a, b), M.psnr_ref(a, b, defect)
                dp = 0.0 if p0 == p1 else abs(p1 - p0)
                if ds > 1e-9 or dp > 1e-6:
                    caught.append((gname, kind, ds, dp))
                break                                             # (the first block of a frame is enough here)
    print(f"[model] N1 defect {defect}: {len(caught)} (geometry, pair) combinations fail, e.g. {caught[:3]}")
    assert caught, defect
