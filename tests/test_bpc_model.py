"""CPU: the NumPy model of the defective-pixel kernels (tests/bpc_model.py) against first principles -- its median against np.median over
explicitly padded CFA planes, its list mode against a literal transcription of the reference's three steps (utils/isp_ops.py:152-160),
and the statistical behaviour of the detection rule on seeded frames.

Counts of the rule on the defect-free frame synthetic.synth_clean(1536, 2048) * 0.6 with Poisson-Gaussian noise on a 959 DN scale,
np.random.default_rng(7), with the TRUE noise model (beta1 = K / 959, beta2 = (sigma / 959)^2), as this model produces them
(3,145,728 pixels; t = 6 is the contract, and all six counts are asserted as they stand here):
    K, sigma = 2, 8:   t = 4: 3     t = 5: 0    t = 6: 0
    K, sigma = 4, 6:   t = 4: 11    t = 5: 0    t = 6: 0
"""
import numpy as np
import pytest

import bpc_model as M
from yond_public_amd import synthetic as S

SCALE = 959.0


def _pg(clean, K, sigma, seed):
    rng = np.random.default_rng(seed)
    return ((rng.poisson(clean * SCALE / K) * K + rng.normal(0.0, sigma, clean.shape)) / SCALE).astype(np.float32)


def _plane_median(plane):
    """cv2.medianBlur(plane, 3) restated: np.median over the 3x3 windows of the edge-padded plane."""
    h, w = plane.shape
    pad = np.pad(plane, 1, mode='edge')
    win = np.stack([pad[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)])
    return np.median(win, axis=0).astype(plane.dtype)


def _reference_steps(raw, bad_points):
    """utils/isp_ops.py:152-160, line for line, with _plane_median for cv2.medianBlur(., 3)."""
    raw = raw.copy()
    H, W = raw.shape
    fixed_raw = raw.reshape(H // 2, 2, W // 2, 2).transpose(0, 2, 1, 3).reshape(H // 2, W // 2, 4).copy()      # bayer2rggb
    for i in range(4):
        fixed_raw[:, :, i] = _plane_median(fixed_raw[:, :, i])
    fixed_raw = fixed_raw.reshape(H // 2, W // 2, 2, 2).transpose(0, 2, 1, 3).reshape(H, W)                     # rggb2bayer
    for p in bad_points:
        raw[p[0], p[1]] = fixed_raw[p[0], p[1]]
    return raw


@pytest.mark.parametrize("shape", [(2, 2), (2, 6), (6, 2), (4, 4), (10, 14), (34, 22)])
def test_median_is_np_median_of_padded_planes(shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    frame = rng.normal(0.3, 0.1, shape).astype(np.float32)
    want = np.empty_like(frame)
    for dy in range(2):
        for dx in range(2):
            want[dy::2, dx::2] = _plane_median(frame[dy::2, dx::2])
    got = M.median9(frame)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    nb = M.neighbourhood(frame)
    assert np.array_equal(nb[4], frame)


def test_list_mode_is_the_reference_transcription():
    rng = np.random.default_rng(3)
    frame = rng.normal(0.3, 0.1, (20, 26)).astype(np.float32)
    pts = np.array([[0, 0], [0, 25], [19, 0], [19, 25], [7, 9], [7, 11], [7, 9], [8, 9], [12, 1]])      # neighbours, a duplicate, corners
    want = _reference_steps(frame, pts)
    got = M.repair_list(frame, pts)
    assert np.array_equal(got, want)
    # neighbouring listed points are repaired from the originals, and nothing else moves
    m = M.median9(frame)
    assert got[7, 9] == m[7, 9] and got[7, 11] == m[7, 11]
    mask = np.zeros(frame.shape, bool)
    mask[pts[:, 0], pts[:, 1]] = True
    assert np.array_equal(got[~mask], frame[~mask])
    # points outside the frame are dropped
    assert np.array_equal(M.repair_list(frame, np.concatenate([pts, [[-1, 3], [20, 0], [3, 26]]])), want)
    assert np.array_equal(M.repair_list(frame, np.zeros((0, 2), int)), frame)


def test_all_border_frames_flag_nothing_at_2x2():
    frame = np.array([[0.1, 5.0], [-3.0, 0.2]], np.float32)              # every pixel is its own nine neighbours
    hot, cold = M.detect(frame, 1e-3, 1e-6, 3.0)
    assert not hot.any() and not cold.any()
    out, info = M.detect_and_repair(frame, 1e-3, 1e-6, 3.0)
    assert np.array_equal(out, frame) and info['hot'] == info['cold'] == 0 and info['points'].shape == (0, 2)


@pytest.mark.parametrize("K,sigma", [(2.0, 8.0), (4.0, 6.0)])
def test_defect_free_frame_flags_nothing_at_t6(K, sigma):
    clean = S.synth_clean(1536, 2048) * 0.6
    noisy = _pg(clean, K, sigma, 7)
    beta1, beta2 = K / SCALE, (sigma / SCALE) ** 2
    counts = {}
    for t in (4.0, 5.0, 6.0):
        hot, cold = M.detect(noisy, beta1, beta2, t)
        counts[t] = int(hot.sum()) + int(cold.sum())
    print(f"[bpc model] K={K}, sigma={sigma}: flagged of {noisy.size} at t=4/5/6: {counts[4.0]}/{counts[5.0]}/{counts[6.0]}")
    assert counts[6.0] == 0                                              # the contract
    # the seeded frame's counts as the model produces them (np.random.default_rng(7), PCG64: Generator.poisson and .normal in this order)
    assert (counts[4.0], counts[5.0], counts[6.0]) == {(2.0, 8.0): (3, 0, 0), (4.0, 6.0): (11, 0, 0)}[(K, sigma)]


@pytest.mark.parametrize("t", [3.0, 6.0])
def test_isolated_defects_above_the_bound_are_all_flagged(t):
    from yond_public_amd import bpc as BP
    K, sigma = 4.0, 6.0
    clean = S.synth_clean(256, 384) * 0.6
    noisy = _pg(clean, K, sigma, 11)
    beta1, beta2 = K / SCALE, (sigma / SCALE) ** 2
    sites = BP.defect_sites(noisy.shape, 60, 5)
    bound = M.certain_bound(noisy.max(), beta1, beta2, t)
    frame = noisy.copy()
    levels = np.float32(bound) * (1.0 + np.float32(1e-3) * (1 + np.arange(len(sites), dtype=np.float32)))       # all above the bound, by 0.1 % and more
    assert (levels.astype(np.float64) > bound).all()
    frame[sites[:, 0], sites[:, 1]] = levels
    hot, cold = M.detect(frame, beta1, beta2, t)
    assert hot[sites[:, 0], sites[:, 1]].all()                           # 100 %: it follows from the rule
    # the repair puts a value of the undisturbed frame there, and nothing that was not flagged moves
    out, info = M.detect_and_repair(frame, beta1, beta2, t)
    assert (out[sites[:, 0], sites[:, 1]] <= noisy.max()).all()
    flagged = hot | cold
    assert np.array_equal(out[~flagged], frame[~flagged]) and info['hot'] == int(hot.sum()) and info['cold'] == int(cold.sum())
    assert {tuple(p) for p in sites} <= {tuple(p) for p in info['points']}
    # cold: zeros under a bright neighbourhood, far below lo - t * sqrt(beta1 * lo + beta2)
    bright = np.argwhere(noisy[2:-2, 2:-2] > 0.45) + 2
    y, x = bright[len(bright) // 2]
    frame2 = noisy.copy()
    frame2[y, x] = 0.0
    hot2, cold2 = M.detect(frame2, beta1, beta2, t)
    assert cold2[y, x] and not hot2[y, x]


def test_touching_same_colour_pair_hides():
    clean = S.synth_clean(64, 64) * 0.6
    noisy = _pg(clean, 4.0, 6.0, 13)
    frame = noisy.copy()
    frame[20, 30] = frame[20, 32] = 2.0
    hot, cold = M.detect(frame, 4.0 / SCALE, (6.0 / SCALE) ** 2, 6.0)
    assert not hot[20, 30] and not hot[20, 32]                           # the stated limit of the rule: each is the other's `hi`
    fixed = M.repair_list(frame, [[20, 30], [20, 32]])                   # a list handles the pair, from the originals
    assert fixed[20, 30] < 1.0 and fixed[20, 32] < 1.0
