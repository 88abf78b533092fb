"""TEST INFRASTRUCTURE ONLY -- write tests/golden/fbinet.npz by running the reference's FBI_Net (archs/comp.py:264-648) on CPU.

Run where the reference tree exists (not on the GPU box):

    python tools/gen_golden_fbinet.py

It imports the reference under the stub modules of `oracle/_refimport.py` (used as is).  The reference's constructors call `.cuda()`
on every layer (archs/comp.py:268, 281, 294, 307, ...): for the run, `torch.nn.Module.cuda` and `torch.Tensor.cuda` return `self`, so
the network is built and run on the CPU, in float32 and -- by `.double()`; the float32 masks promote -- in float64.  The file stores
OUTPUTS, seeds and key lists only; the weights and inputs are regenerated from the seeds by tests/fbinet_common.py:
  - cases (a)-(e) (tests/fbinet_common.CASES) in float32 (`y32_*`) and in float64 (`d64_*`: the float64 output minus the float32 one,
    stored as float32 -- the scale of the reference's own rounding);
  - `dn_vst`: the reference's own VST_Denoiser (YOND_SIDD.py:250-299, on `object.__new__(ref.YOND_SIDD)` as oracle/gen_golden.py does)
    with denoiser='fbi', bias_corr='pre', net (a) with weakly denoising weights, on the 96 x 128 Poisson-Gaussian Bayer frame of
    the DnCNN fixture (K = 4, sigma = 6);
  - the state_dict keys and shapes of (a) and (c).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import _refimport  # noqa: E402
import fbinet_common as D  # noqa: E402
from gen_golden_estnet import save_npz  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "fbinet.npz")
W_SEED, X_SEED, VST_SEED = 20261022, 5200, 78
REF_KEYS = ('channel', 'output_channel', 'nf', 'mul', 'num_of_layers', 'case', 'output_type', 'sigmoid_value', 'res')


def ref_net(ref, args, sd, dtype=torch.float32):
    net = ref.FBI_Net({k: args[k] for k in REF_KEYS})
    tensors = {k: torch.as_tensor(v).clone() for k, v in sd.items()}
    ref.load_weights(net, tensors, by_name=False)
    net.load_state_dict(tensors)                                                # strict, too
    return net.to(dtype).eval()


def main():
    torch.set_num_threads(8)
    ref = _refimport.import_reference()
    torch.nn.Module.cuda = lambda self, *a, **k: self
    torch.Tensor.cuda = lambda self, *a, **k: self
    out = {"w_seed": np.int64(W_SEED), "x_seed": np.int64(X_SEED), "vst_seed": np.int64(VST_SEED)}
    keys = []
    for name, (args, shape) in D.CASES.items():
        sd = D.weights(args, D.case_seed(W_SEED, name))
        x = D.case_input(shape, D.case_seed(X_SEED, name))
        net = ref_net(ref, args, sd)
        if name in ('a', 'c'):
            keys += [f"{name}:{k}:{'x'.join(map(str, v.shape))}" for k, v in net.state_dict().items()]
        with torch.no_grad():
            y32 = net(x.clone())
            y64 = ref_net(ref, args, sd, torch.float64)(x.double())
        assert float(y64.abs().max()) < 100.0, (name, float(y64.abs().max()))
        out[f"y32_{name}"] = y32.numpy().astype(np.float32)
        out[f"d64_{name}"] = (y64 - y32.double()).numpy().astype(np.float32)
        print(f"{name}: {tuple(shape)} max|y64| {float(y64.abs().max()):.3f}  max|y32 - y64| {float((y64 - y32.double()).abs().max()):.3e}", flush=True)
    # dn_vst
    args, _ = D.CASES['a']
    sd = D.vst_weights(args, VST_SEED)
    obj = object.__new__(ref.YOND_SIDD)
    obj.biaslut = None
    obj.device = torch.device('cpu')
    obj.arch = {k: args[k] for k in REF_KEYS}
    obj.net = ref_net(ref, args, sd)
    obj.pipe = {'vst_type': 'exact'}
    obj.dst = {'root_dir': '/nonexistent'}
    obj.args, obj.est_args, obj.est_net, obj.logfile = {}, {}, {}, None
    dn = ref.YOND_SIDD.VST_Denoiser(obj, D.vst_frame(), None, 'pre', None, denoiser='fbi', p=D.vst_params())
    out["dn_vst"] = np.asarray(dn)
    noisy = D.vst_frame()
    print(f"dn_vst: {np.asarray(dn).shape} {np.asarray(dn).dtype}  mean |dn - noisy| {float(np.abs(np.asarray(dn) - noisy).mean()):.4f}", flush=True)
    out["keys"] = np.array(keys)
    save_npz(OUT, out)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
