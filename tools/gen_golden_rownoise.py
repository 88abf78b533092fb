"""TEST INFRASTRUCTURE ONLY -- write tests/golden/rownoise.npz by running the reference's row_denoise.

Run where the reference tree exists (not on the GPU box):

    python tools/gen_golden_rownoise.py

It imports the reference under the stub modules of `oracle/_refimport.py` (used as is), then sets `cv2.BORDER_REPLICATE` and
`cv2.bilateralFilter` on the stub module object to the restated 1-D filter of tests/rownoise_model.py (OpenCV is absent: the filter
is UNPINNED, everything around it -- the row split, the means, the sign, the reassembly -- is the reference's own code), and calls the
reference's own row_denoise(None, iso, data=...) (utils/isp_algos.py:319-334) on the seeded frames of rownoise_model.GOLDEN.  Seeds,
parameters and OUTPUTS only are stored: the tests rebuild the inputs from the seeds.

Seen when this was written: with float64 `data` the reference and the float64 model differ by at most 3.4e-13 on the 60 x 96 frame (the
model evaluates the offset in its difference form, the stub in the literal one);
with float32 `data` they differ by the reference's float32 mean (3.1e-5 at level 500).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _refimport  # noqa: E402
import rownoise_model as M  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "rownoise.npz")


def main():
    ref = _refimport.import_reference()
    cv2 = sys.modules["cv2"]
    assert getattr(cv2, "__stub__", False)
    cv2.BORDER_REPLICATE = 1
    cv2.bilateralFilter = M.cv2_bilateral_1d
    out, names = {}, []
    for name, (seed, H, W, kw, dtype, iso) in M.GOLDEN.items():
        x, _ = M.golden_frame(name)
        got = np.asarray(ref.row_denoise(None, iso, data=x.copy()))
        assert got.shape == (H, W) and got.dtype == np.float64
        names.append(name)
        out[name + "_out"] = got
        out[name + "_params"] = np.array([seed, H, W, iso], np.int64)
        out[name + "_dtype"] = np.array(np.dtype(dtype).name)
        want = M.row_denoise_f64(x, iso)
        with np.errstate(invalid='ignore'):
            dist = np.abs(got - want)
        print(f"{name}: {H} x {W} {np.dtype(dtype).name}, iso {iso}: max |reference - model| = {np.nanmax(dist):.3e}, "
              f"{int(np.isnan(got).sum())} NaN in the reference's output")
    out["cases"] = np.array(names)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KiB): {len(names)} row_denoise cases")


if __name__ == "__main__":
    main()
