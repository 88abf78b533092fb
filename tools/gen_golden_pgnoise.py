"""TEST INFRASTRUCTURE ONLY -- write tests/golden/pgnoise.npz by running the reference's camera-noise prior.

Run where the reference tree exists (not on the GPU box):

    python tools/gen_golden_pgnoise.py

It imports the reference under the stub modules of `oracle/_refimport.py` (used as is), builds DIV2K_PG_Dataset with its parent's
__init__ patched out (no data directory is needed for the prior, and the constants stay the reference's own) and stores NUMBERS
only: for each seed s, get_noise_params() (data_process/yond_datasets.py:672-682) right after np.random.seed(s), plus the prior's
constants.  tests/test_pgnoise_host.py replays them through yond_public_amd.pgnoise.sample_pg_params.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import _refimport  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pgnoise.npz")
SEEDS = (0, 1, 2, 3, 7, 1997, 20261018, 2 ** 32 - 1)
FIELDS = ("K", "sigma", "beta1", "beta2", "wp", "bl", "scale")


def main():
    _refimport.import_reference()
    import data_process.yond_datasets as yd
    parent = yd.DIV2K_PG_Dataset.__mro__[1]
    init = parent.__init__
    parent.__init__ = lambda self, args=None: None
    try:
        ds = yd.DIV2K_PG_Dataset(None)
    finally:
        parent.__init__ = init
    out = {"seeds": np.array(SEEDS, np.int64)}
    for s in SEEDS:
        np.random.seed(s)
        p = ds.get_noise_params()
        assert sorted(p) == sorted(FIELDS), sorted(p)
        out[f"params_{s}"] = np.array([p[f] for f in FIELDS], np.float64)
    out["fields"] = np.array(FIELDS)
    out["prior_names"] = np.array(sorted(ds.noise_params))
    out["prior_values"] = np.array([ds.noise_params[k] for k in sorted(ds.noise_params)], np.float64)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes): {len(SEEDS)} seeds")


if __name__ == "__main__":
    main()
