"""CPU: the NumPy model of the row-noise removal (tests/rownoise_model.py) against the reference's row_denoise as recorded in
tests/golden/rownoise.npz (tools/gen_golden_rownoise.py: the reference's own code around the restated 1-D bilateral filter), and every
single-defect variant against the model: a variant that the GPU tests' bound cannot tell from the model tests nothing."""
import os

import numpy as np
import pytest

import rownoise_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "rownoise.npz"), allow_pickle=False)


def test_fixture_lists_the_models_cases(golden):
    assert list(golden["cases"]) == list(M.GOLDEN)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "rownoise.npz")) < 100 * 1024
    for name, (seed, H, W, kw, dtype, iso) in M.GOLDEN.items():
        assert golden[name + "_params"].tolist() == [seed, H, W, iso] and str(golden[name + "_dtype"]) == np.dtype(dtype).name
        assert golden[name + "_out"].shape == (H, W) and golden[name + "_out"].dtype == np.float64 and max(H, W) <= 96


@pytest.mark.parametrize("name", list(M.GOLDEN))
def test_model_equals_the_reference(golden, name):
    x, iso = M.golden_frame(name)
    ref = golden[name + "_out"]
    got = M.row_denoise_f64(x, iso)
    H, W = x.shape
    rows = np.ones(H, bool)
    if 'nan' in name:
        # the reference has no containment: the NaN pixel's row and every row of its parity within the window are NaN there.  The
        # model must equal it on every other row, and be finite everywhere but at the pixel itself
        y0 = M.GOLDEN_NAN_AT[0]
        rows = ~np.isnan(ref).any(axis=1)
        want_nan = np.array([(y % 2 == y0 % 2) and abs(y - y0) // 2 <= 12 for y in range(H)])
        assert np.array_equal(~rows, want_nan) and rows.sum() >= H // 2 + 4
        only = np.zeros((H, W), bool)
        only[M.GOLDEN_NAN_AT] = True
        assert np.array_equal(np.isnan(got), only)
        spread = M.row_denoise_f64(x, iso, defect='nan_spreads')
        assert np.array_equal(np.isnan(spread), np.isnan(ref))         # ... and without containment the model is the reference
    if x.dtype == np.float64:
        bound = 1e-9
    else:
        bound = W * 2.0 ** -24 * float(np.abs(x).max())                  # the reference's float32 mean
    dist = float(np.abs(got[rows] - ref[rows]).max())
    print(f"[rownoise model] {name}: max |model - reference| = {dist:.3e} (bound {bound:.3e})")
    assert dist <= bound


def _cases_for(defect):
    """(name, per) pairs on which `defect` can show at all."""
    if defect == 'plane_swapped':
        return [(n, M.PLANE) for n in M.GOLDEN if 'nan' not in n]
    if defect == 'nan_spreads':
        return [(n, per) for n in M.GOLDEN if 'nan' in n for per in (M.ROW, M.PLANE)]
    return [(n, M.ROW) for n in M.GOLDEN if 'nan' not in n]


@pytest.mark.parametrize("defect", M.DEFECTS)
def test_every_defect_is_outside_the_gpu_bound(defect):
    """On at least one stored case the variant's float32 output is further from the model's float64 value than the GPU test's end-to-end
    bound, half a float32 ulp plus e2e_band."""
    seen = []
    for name, per in _cases_for(defect):
        x, iso = M.golden_frame(name)
        x = x.astype(np.float32)
        ss = 1.0 + iso / 200.0
        _, _, z = M.row_denoise(x, per, 25, 10.0, ss)
        bad, _, _ = M.row_denoise(x, per, 25, 10.0, ss, defect=defect)
        band = M.per_pixel(M.e2e_band(x, per, 25, 10.0, ss), x.shape[1])
        with np.errstate(invalid='ignore'):
            excess = np.abs(bad.astype(np.float64) - z) - (0.5 * np.spacing(np.abs(bad)).astype(np.float64) + band)
        differs = bool((np.isnan(bad) != np.isnan(z)).any()) or float(np.nanmax(excess)) > 0
        seen.append((name, per, differs, float(np.nanmax(excess))))
    print(f"[rownoise model] {defect}: " + ", ".join(f"{n}/{p}: {'told apart' if d else 'NOT told apart'} ({e:.2e})" for n, p, d, e in seen))
    assert any(d for _, _, d, _ in seen)


def test_the_step_case_needs_the_range_weight():
    """The 80-unit edge of g2 is more than 3 sigma_color: without the range weight the rows next to it move by units."""
    x, iso = M.golden_frame('g2_step_52x16')
    ss = 1.0 + iso / 200.0
    _, off, _ = M.row_denoise(x.astype(np.float32), M.ROW, 25, 10.0, ss)
    _, off_nr, _ = M.row_denoise(x.astype(np.float32), M.ROW, 25, 10.0, ss, defect='no_range_weight')
    mid = slice(52 // 2 - 4, 52 // 2 + 4)
    assert np.abs(off[mid]).max() < 12 and np.abs(off_nr[mid] - off[mid]).max() > 10


def test_exact_zero_offsets():
    """d = 1, and one row per parity: the offset is exactly 0 and the output is the input, bit for bit."""
    x = M.frame(7, 8, 12).astype(np.float32)
    for per in (M.ROW, M.PLANE):
        out, off, _ = M.row_denoise(x, per, 1, 10.0, 9.0)
        assert (off == 0).all() and np.array_equal(out.view(np.uint32), x.view(np.uint32))
        out, off, _ = M.row_denoise(x[:2], per, 25, 10.0, 9.0)
        assert (off == 0).all() and np.array_equal(out.view(np.uint32), x[:2].view(np.uint32))


def test_bands_are_small_and_positive():
    x = M.frame(8, 52, 16).astype(np.float32)
    sums = M.row_sums(x)
    b2 = M.offset_band(sums, 16, M.ROW, 25, 10.0, 9.0)
    b4 = M.e2e_band(x, M.ROW, 25, 10.0, 9.0)
    assert (b2 >= 0).all() and (b4 >= b2).all() and b2.max() < 1e-12 and b4.max() < 1e-10
    assert (M.sums_bound(x) > 0).all() and M.sums_bound(x).max() < 1e-11
