"""TEST INFRASTRUCTURE ONLY -- write tests/golden/noisekld.npz by running the reference's get_histogram / cal_kld.

Run where the reference tree exists (not on the GPU box):

    python tools/gen_golden_noisekld.py

It imports the reference under the stub modules of `oracle/_refimport.py` (used as is), runs utils/sidd_utils.py:280-304 on the seeded
cases of tests/noisekld_model.py and stores DATA only, per case <name>:
  - <name>_p, <name>_q            the float32 inputs (functions of the case's name alone: make_case reproduces them);
  - <name>_hist_p, <name>_hist_q  the reference's get_histogram output on cal_kld's edges (float64, counts / n);
  - <name>_kld                    the reference's cal_kld (kl_fwd, float64);
and `edges`, the reference's own edge array.  Before it writes, it asserts what tests/test_noisekld_model.py asserts: the model's counts
equal the reference's hist * n exactly and its KLD is within the derived bound on every case, and every defect variant breaks at least
one case -- the fixture cannot go slack.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _refimport  # noqa: E402
import noisekld_model as M  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "noisekld.npz")


def main():
    _refimport.import_reference()
    import importlib
    ref = importlib.import_module("utils.sidd_utils")
    ref_edges = np.concatenate(([-1000.0], np.arange(-0.1, 0.1 + 1e-9, 0.2 / 64), [1000.0]), axis=0)     # cal_kld's own call (:292-293)
    assert ref_edges.tobytes() == M.edges().tobytes()
    out = {"names": np.array(list(M.CASES)), "edges": ref_edges}
    broken = {d: [] for d in M.DEFECTS}
    for name in M.CASES:
        p, q = M.make_case(name)
        with np.errstate(invalid='ignore'):
            hp, _ = ref.get_histogram(p, ref_edges)
            hq, _ = ref.get_histogram(q, ref_edges)
            kl = float(ref.cal_kld(p, q))
        cp, cq = M.hist_counts(p), M.hist_counts(q)
        assert np.array_equal(cp, np.rint(hp * p.size)) and np.array_equal(cq, np.rint(hq * q.size)), name
        assert np.array_equal(cp / p.size, hp) and np.array_equal(cq / q.size, hq), name
        bound = M.kld_bound(cp, cq, p.size, q.size)
        assert abs(M.cal_kld(p, q) - kl) <= bound, (name, M.cal_kld(p, q), kl, bound)
        for d in M.DEFECTS:
            e = M.edges(defect=d)
            same = np.array_equal(M.hist_counts(p, e, d), cp) and np.array_equal(M.hist_counts(q, e, d), cq)
            if not same or not abs(M.cal_kld(p, q, defect=d) - kl) <= bound:
                broken[d].append(name)
        out[f"{name}_p"], out[f"{name}_q"], out[f"{name}_hist_p"], out[f"{name}_hist_q"] = p, q, hp, hq
        out[f"{name}_kld"] = np.float64(kl)
        print(f"{name}: p {p.shape}, q {q.shape}, counted {int(cp.sum())}/{p.size} and {int(cq.sum())}/{q.size}, kl_fwd {kl:.6e}, bound {bound:.2e}")
    for d, names in broken.items():
        print(f"defect {d}: breaks {names}")
        assert names, d
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
