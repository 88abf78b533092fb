"""TEST INFRASTRUCTURE ONLY -- write tests/golden/illum.npz by running the reference's IlluminanceCorrect.

Run where the reference tree exists (not on the GPU box):

    python tools/gen_golden_illum.py

It imports the reference under the stub modules of `oracle/_refimport.py` (used as is), runs data_process/__init__.py:140-171
(IlluminanceCorrect.forward, on the CPU, one thread) on the seeded cases of tests/illum_model.py and stores DATA only, per case <name>:
  - <name>_pred, <name>_source   the float32 inputs (functions of the case's seed alone: make_case reproduces them);
  - <name>_out                   the reference's float32 output;
  - <name>_gain_dist             per item, the relative distance of the reference's gain (read back as out / clamp(pred) is not exact:
                                 it is recomputed with the reference's own two float32 dots) from the float64 model's -- the measured
                                 value the GPU test's tolerance against these outputs is built from.
Before it writes, it asserts what tests/test_illum_model.py asserts: the model is within the derived bound of the reference on every
case and every defect variant is outside it on every case that exercises it -- the fixture cannot go slack.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _refimport  # noqa: E402
import illum_model as M  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "illum.npz")


def main():
    import torch
    torch.set_num_threads(1)
    _refimport.import_reference()
    import importlib
    cls = importlib.import_module("data_process").IlluminanceCorrect
    mod = cls()
    out = {"names": np.array(list(M.CASES))}
    for name in M.CASES:
        pred, source = M.make_case(name)
        tp, ts = torch.from_numpy(pred), torch.from_numpy(source)
        with torch.no_grad():
            ref = mod(tp, ts).numpy().astype(np.float32)
            again = mod(tp.clone(), ts.clone()).numpy()
        assert ref.tobytes() == again.tobytes(), name
        dist = []
        for i in range(pred.shape[0]):
            s = source[i if source.shape[0] != 1 else 0]
            with torch.no_grad():                                     # the reference's own expression for the scalar (:160-168)
                p = torch.clamp(tp[i:i + 1], 0, 1)
                src = torch.from_numpy(s[None])
                pc, sc = p[src != 1], src[src != 1]
                g_ref = float(torch.dot(pc, sc) / torch.dot(pc, pc))
            ms = M.sums(pred[i], s)
            g_model = ms[4, 0] / ms[4, 1]
            dist.append(abs(g_ref - g_model) / abs(g_model))
            n_incl = int(ms[4, 2])
            model = M.apply(pred[i], ms)
            M.assert_within(ref[i], model, M.out_bound(n_incl), f"{name}[{i}] model")
        for d in M.DEFECTS:
            if M.exercises(name, d):
                M.assert_outside(ref, M.forward(pred, source, defect=d), pred, source, f"{name} {d}")
        out[f"{name}_pred"], out[f"{name}_source"], out[f"{name}_out"] = pred, source, ref
        out[f"{name}_gain_dist"] = np.array(dist, np.float64)
        print(f"{name}: predict {pred.shape}, source {source.shape}, gain distance {['%.3e' % v for v in dist]}")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
