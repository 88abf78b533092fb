"""TEST INFRASTRUCTURE ONLY -- write tests/golden/camnoise.npz by running the reference's camera-noise parameter prior and model.

Run where the reference tree exists (not on the GPU box):

    python tools/gen_golden_camnoise.py

It imports the reference under the stub modules of `oracle/_refimport.py` (used as is) and stores DATA only: what the reference's
functions return or draw while they run.
  - table_<camera>_names / _values: the dicts get_camera_noisy_params (data_process/process.py) returns for SonyA7S2_lowISO,
    SonyA7S2_highISO and CRVD;
  - CRVD_K_points / CRVD_log_sigGs_points: the five ISO points sample_params (process.py:394-452) takes for CRVD, as it hands them
    on: K is the returned K per point; log sigGs is the `loc` it passes to np.random.normal for sigGs (recorded by a wrapper around
    np.random.normal while sample_params runs with np.random.randint pinned to each point in turn);
  - params_<camera>_<ln>_<seed>: the dict sample_params returns after np.random.seed(seed), seed 0..7, ln_ratio False / True, in the
    order of `fields`.  The seeds must reach both ISO branches of the Sony and more than one CRVD point (asserted);
  - obs_<code>: generate_noisy_obs (process.py:631-671) on a constant [4][6][8] plane with K = 1e-12, sigGs = 0 and codes r, rq,
    rqd: which axes the row and bias terms vary along.
tests/test_camnoise_host.py replays the draws on the CPU, tests/test_hip_camnoise.py compares the kernel's structure.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import _refimport  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "camnoise.npz")
FIELDS = ["K", "sigTL", "sigR", "sigGs", "bias", "lam", "q", "ratio", "wp", "bl"]
SEEDS = list(range(8))


def main():
    _refimport.import_reference()
    pr = sys.modules["data_process.process"]          # (the attribute of that name on the package is shadowed by a function)
    out = {"fields": np.array(FIELDS), "seeds": np.array(SEEDS, np.int64)}
    for cam in ("SonyA7S2_lowISO", "SonyA7S2_highISO", "CRVD"):
        t = pr.get_camera_noisy_params(camera_type=cam)
        out[f"table_{cam}_names"] = np.array(list(t))
        out[f"table_{cam}_values"] = np.array([t[k] for k in t], np.float64)

    # the CRVD points, as sample_params hands them on
    real_normal, real_randint = np.random.normal, np.random.randint
    K_pts, gs_pts = [], []
    try:
        for point in range(5):
            locs = []

            def normal(loc=0.0, scale=1.0, size=None, _locs=locs):
                _locs.append((float(loc), float(scale)))
                return real_normal(loc=loc, scale=scale, size=size)
            np.random.normal = normal
            np.random.randint = lambda *a, _p=point, **k: _p
            p = pr.sample_params(camera_type="CRVD")
            t = pr.get_camera_noisy_params(camera_type="CRVD")
            K_pts.append(float(p["K"]))
            gs = [loc for loc, scale in locs if scale == t["sigGssig"]]
            assert len(gs) == 1, locs
            gs_pts.append(gs[0])
    finally:
        np.random.normal, np.random.randint = real_normal, real_randint
    out["CRVD_K_points"] = np.array(K_pts, np.float64)
    out["CRVD_log_sigGs_points"] = np.array(gs_pts, np.float64)

    branches = {"SonyA7S2": set(), "CRVD": set()}
    for cam in ("SonyA7S2", "CRVD"):
        for ln in (False, True):
            for s in SEEDS:
                np.random.seed(s)
                p = pr.sample_params(camera_type=cam, ln_ratio=ln)
                assert sorted(p) == sorted(FIELDS)
                out[f"params_{cam}_{int(ln)}_{s}"] = np.array([p[f] for f in FIELDS], np.float64)
                branches[cam].add(float(p["lam"]) if cam == "SonyA7S2" else float(p["K"]))
    assert len(branches["SonyA7S2"]) == 2, "the seeds reach one ISO branch only: add seeds"
    assert len(branches["CRVD"]) >= 3, "the seeds reach too few CRVD points: add seeds"

    clean = np.full((4, 6, 8), 0.25, np.float32)
    param = {"K": 1e-12, "sigTL": 0.0, "sigR": 2.0, "sigGs": 0.0, "bias": np.array([1.0, -2.0, 3.0, 0.5]), "lam": 0.0, "q": 1 / 2 ** 10,
             "ratio": 1.0, "wp": 1023, "bl": 64}
    for code in ("r", "rq", "rqd"):
        np.random.seed(11)
        out[f"obs_{code}"] = pr.generate_noisy_obs(clean, noise_code=code, param=dict(param)).astype(np.float32)
    out["obs_clean"] = clean
    out["obs_param_names"] = np.array([k for k in param if k != "bias"])
    out["obs_param_values"] = np.array([param[k] for k in param if k != "bias"], np.float64)
    out["obs_bias"] = param["bias"]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
