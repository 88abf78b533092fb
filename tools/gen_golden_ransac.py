"""TEST INFRASTRUCTURE ONLY -- write tests/golden/ransac.npz by running the reference's polyfit(x, y, ransac=True).

Run where the reference tree and scikit-learn exist (not on the GPU box):

    python tools/gen_golden_ransac.py

It imports the reference under the stub modules of `oracle/_refimport.py` (used as is), feeds utils/isp_algos.py:345-362 the synthetic
point sets of tests/ransac_model.py (functions of np.random.RandomState(seed) alone) and stores RESULTS only, per case <name>:
  - <name>_res        (slope, intercept) as polyfit returns them (float64);
  - <name>_n_inliers  inlier_mask_.sum() of the fitted RANSACRegressor, <name>_n_trials its n_trials_ -- captured by a recording
                      subclass put in place of lm.RANSACRegressor while polyfit runs;
  - <name>_thr        the residual threshold sklearn derives, np.median(np.abs(y - np.median(y))) on the float32 y it is handed;
  - <name>_n, <name>_m  points after the non-saturation rule and min_samples;
  - <name>_seed       the RandomState seed of the point set.
No point arrays are stored.  tests/test_ransac_model.py holds the NumPy model to these, tests/test_hip_ransac.py the kernels.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _refimport  # noqa: E402
import ransac_model as RM  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ransac.npz")


def main():
    _refimport.import_reference()
    algos = sys.modules["utils.isp_algos"]
    lm = algos.lm
    seen = []

    class Recording(lm.RANSACRegressor):
        def fit(self, X, y, **kw):
            out = super().fit(X, y, **kw)
            seen.append(dict(n_inliers=int(self.inlier_mask_.sum()), n_trials=int(self.n_trials_), n=int(len(y)), m=int(self.min_samples),
                             thr=np.median(np.abs(y - np.median(y))), y_dtype=str(y.dtype)))
            return out

    real = lm.RANSACRegressor
    out = {"names": np.array(list(RM.CASES))}
    try:
        lm.RANSACRegressor = Recording
        for name, case in RM.CASES.items():
            x, y = RM.make_points(name)
            res = algos.polyfit(x, y, ransac=True)
            rec = seen.pop()
            assert not seen and rec["y_dtype"] == "float32", rec
            again = algos.polyfit(x, y, ransac=True)                       # setup_seed(2024) inside: deterministic
            assert tuple(again) == tuple(res), (name, res, again)
            seen.clear()
            out[f"{name}_res"] = np.array(res, np.float64)
            out[f"{name}_n_inliers"] = np.int64(rec["n_inliers"])
            out[f"{name}_n_trials"] = np.int64(rec["n_trials"])
            out[f"{name}_thr"] = np.float32(rec["thr"])
            out[f"{name}_n"] = np.int64(rec["n"])
            out[f"{name}_m"] = np.int64(rec["m"])
            out[f"{name}_seed"] = np.int64(case["seed"])
            print(f"{name}: res={tuple(res)}, inliers {rec['n_inliers']} of {rec['n']}, m={rec['m']}, trials {rec['n_trials']}, thr={rec['thr']!r}")
    finally:
        lm.RANSACRegressor = real
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
