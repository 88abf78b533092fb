"""CPU: tests/isp_model.py (the float64 model of yond_render_srgb) against tests/golden/isp.npz -- the reference's own
process_sidd_image / FastISP around the restated demosaic (tools/gen_golden_isp.py)."""
import numpy as np
import pytest

import isp_model as M


@pytest.fixture(scope="module")
def g(golden):
    return golden("isp")


def test_model_codes_equal_the_reference_outside_the_band(g):
    assert len(g["sidd_cases"]) == 8
    for c in g["sidd_cases"]:
        codes, x = M.render_sidd(g[c + "_frame"], g[c + "_pattern"], g["wb"], g["cst"])
        want = g[c + "_bgr"]
        assert want.dtype == np.uint8 and want.shape == codes.shape
        n = M.check_codes(codes[..., ::-1], want, x[..., ::-1], c)               # the reference returns BGR
        print(f"[isp] {c}: {codes.shape}, {n} codes differ (all inside the band), {int(M.in_band(x).sum())} of {x.size} in the band")


def test_scene_holds_white_and_black_and_the_four_patterns(g):
    """What the cases are there for: saturation at both ends, every flip, and the reference's white = 254 where cam2rgb's row sums to 1 - eps."""
    pats = {tuple(g[f"scene_{p}_pattern"].reshape(-1)) for p in ("rggb", "grbg", "gbrg", "bggr")}
    assert pats == {(1, 2, 2, 3), (2, 1, 3, 2), (2, 3, 1, 2), (3, 2, 2, 1)}
    img = g["scene_rggb_bgr"]
    assert (img >= 254).all(axis=-1).any() and (img == 0).all(axis=-1).any()
    assert (img == 254).any(), "a white element whose row of cam2rgb sums to 1 - 2^-52 renders as 254 in the reference"
    for c in ("crop_2x2", "crop_2x34", "crop_6x10"):
        assert not (g[c + "_bgr"] >= 254).all(axis=-1).any()


def test_tie_case_goes_horizontal(g):
    """A flat frame with one bright pixel: left/right and up/down gradients tie at its four neighbours -> the horizontal mean."""
    q = np.full((12, 12), 100, np.int64)
    q[2, 2] = 900                                                               # an R site
    d = M.demosaic(q)
    assert d[2, 2, 0] == 900 and d[2, 2, 1] == 100                              # gh == gv == 0: (left + right + 1) >> 1
    assert d[3, 3, 0] == (900 + 3 * 100 + 2) >> 2                               # B site: R from the four diagonals
    assert d[2, 3, 0] == (900 + 100 + 1) >> 1 and d[3, 2, 0] == (900 + 100 + 1) >> 1
    assert d[2, 1, 0] == (900 + 100 + 1) >> 1


def test_demosaic_mirrors_without_repeating_the_edge():
    rng = np.random.default_rng(3)
    q = rng.integers(0, 16384, (6, 8))
    big = np.pad(q, 2, mode='reflect')                                          # parity-preserving mirror, applied by hand
    np.testing.assert_array_equal(M.demosaic(q), M.demosaic(big)[2:-2, 2:-2])
    d = M.demosaic(rng.integers(0, 16384, (2, 2)))
    assert d.shape == (2, 2, 3)


def test_float32_quotient_is_the_rounded_double_quotient():
    v = np.arange(16384)
    np.testing.assert_array_equal(v.astype(np.float32) / np.float32(16383), (v / 16383.0).astype(np.float32))


def test_ccm_sum_order_is_numpy_sum():
    rng = np.random.default_rng(5)
    d, m = rng.uniform(0, 1, (64, 3)), rng.normal(0, 1, (3, 3))
    want = np.sum(d[:, None, :] * m[None, :, :], axis=-1)
    got = np.stack([(d[:, 0] * m[r, 0] + d[:, 1] * m[r, 1]) + d[:, 2] * m[r, 2] for r in range(3)], axis=-1)
    np.testing.assert_array_equal(got, want)


def test_model_fastisp_within_4_ulp(g):
    for c in g["fast_cases"]:
        wb, ccm = (g["fast_wb"], g["fast_ccm"]) if c == "fast_given" else (None, None)
        y, _ = M.fast_isp(g["fast_img4c"], wb, ccm)
        want = g[c + "_rgb"]
        assert want.shape == (32, 48, 3) and want.dtype == np.float64
        ulps = np.abs(y - want) / np.spacing(np.maximum(np.abs(want), np.finfo(np.float64).tiny))
        print(f"[isp] {c}: max {ulps.max():.1f} float64 ulp")
        assert ulps.max() <= 4                                                  # NumPy's array pow is not correctly rounded
        assert (want == 1.0).any() and (want == 0.0).any()


def test_band_predicate():
    t = M.thresholds()
    assert M.in_band(t).all() and M.in_band(t * (1 + 2.0 ** -49)).all() and M.in_band(t * (1 - 2.0 ** -49)).all()
    assert not M.in_band(t * (1 + 2.0 ** -46)).any() and not M.in_band(t * (1 - 2.0 ** -46)).any()
    assert not M.in_band(np.array([0.0, 1e-8, 0.5 * (t[100] + t[101])])).any()
