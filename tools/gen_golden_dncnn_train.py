"""TEST INFRASTRUCTURE ONLY -- write tests/golden/dncnn_train.npz by running the reference trainer's own step on its DnCNN, on CPU.

Run where the reference tree exists (not on the GPU box):

    python tools/gen_golden_dncnn_train.py

It imports the reference under the stub modules of `oracle/_refimport.py` (used as is) and stores RESULTS and seeds only; weights and
batches are regenerated from the seed by tests/dncnn_train_common.py.  Per variant (`bn`: use_bn True, `nobn`: False; nf 32, depth 4,
batches of 2 x 4 x 16 x 16) the reference's DnCNN (archs/comp.py:3-33) takes two consecutive steps of trainer_AWGN.py:85-117 --
net.train(); optimizer.zero_grad(); pred = net(lr); loss = Unet_Loss()(pred, hr); loss.backward(); Adam(net.parameters(), lr).step() --
once in float32 and once in float64, then evaluates a third input in .eval() mode.  Stored per step s = 1, 2:
    <v>/loss<s>                 the float32 loss (as float64)          <v>_d64/...: the float64 run minus the float32 one
    <v>/g<s>/<param>            every gradient (dncnn_train_common.sample)     (float32-rounded, as tests/dncnn_common.py stores them)
    <v>/w<s>/<param>            every updated parameter (sampled alike)
    <v>/b<s>/<buffer>           running_mean, running_var, num_batches_tracked of every BatchNorm layer
    <v>/gap_{g,w,b}<s>/<name>   max |float32 - float64| over the WHOLE tensor;   <v>/gmax<s>/<param>: max |gradient| over the whole tensor
    <v>/mask<s>/<i>             the ReLU masks (input of dncnn.<i> > 0), [N][H][W][C] order, np.packbits
and <v>/eval (the eval-mode output after step 2), <v>/seed, <v>/margin.

Condition on the inputs: a ReLU's derivative is discontinuous, so a pre-activation with different signs in the two runs would make
their gradients incomparable.  Seeds are walked from SEED0 until, in both steps, the float32 and float64 masks are identical at every
ReLU and the smallest |pre-activation| is at least 1e-4 of its layer's RMS (dncnn_train_common.MARGIN); both are asserted again on the
stored run."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import _refimport  # noqa: E402
import dncnn_train_common as T  # noqa: E402
from gen_golden_estnet import save_npz  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "dncnn_train.npz")
SEED0 = 20261021
MAX_SEEDS = 200000


def run(ref, name, seed, dtype):
    """Two steps and the evaluation.  Returns (records per step, eval output, pre-activations per step {index: tensor})."""
    net = ref.DnCNN(dict(T.VARIANTS[name]))
    sd = {k: torch.as_tensor(v) for k, v in T.weights(name, seed).items()}
    ref.load_weights(net, sd, by_name=False)
    net = net.to(dtype)
    pres = {}
    for i in T.relu_indices(name):
        assert isinstance(net.dncnn[i], torch.nn.ReLU)
        net.dncnn[i].register_forward_pre_hook(lambda m, inp, i=i: pres.__setitem__(i, inp[0].detach().clone()))
    loss_fn = ref.Unet_Loss()
    opt = torch.optim.Adam(net.parameters(), lr=T.LR)
    steps, acts = [], []
    for k in range(T.STEPS):
        lr_img, hr_img = (t.to(dtype) for t in T.batch(seed, k))
        net.train()
        opt.zero_grad()
        pred = net(lr_img)
        loss = loss_fn(pred, hr_img)
        loss.backward()
        acts.append(dict(pres))
        grads = {n: p.grad.detach().clone() for n, p in net.named_parameters()}
        opt.step()
        steps.append(dict(loss=float(loss.detach()), g=grads, w={n: p.detach().clone() for n, p in net.named_parameters()},
                          b={n: b.detach().clone() for n, b in net.named_buffers()}))
    net.eval()
    pres.clear()
    with torch.no_grad():
        y = net(T.batch(seed, 2)[0].to(dtype))
    return steps, y, acts


def margin(acts):
    """min over steps and ReLUs of min |pre-activation| / RMS(layer)."""
    return min(float(a.abs().min() / a.double().pow(2).mean().sqrt()) for step in acts for a in step.values())


def same_masks(a32, a64):
    return all(torch.equal(s32[i] > 0, s64[i] > 0) for s32, s64 in zip(a32, a64) for i in s32)


def main():
    torch.set_num_threads(8)
    ref = _refimport.import_reference()
    out = {}
    for name in T.VARIANTS:
        for seed in range(SEED0, SEED0 + MAX_SEEDS):
            s32, y32, a32 = run(ref, name, seed, torch.float32)
            if margin(a32) < T.MARGIN:
                continue
            s64, y64, a64 = run(ref, name, seed, torch.float64)
            if margin(a64) >= T.MARGIN and same_masks(a32, a64):
                break
        else:
            raise SystemExit(f"{name}: no seed in {MAX_SEEDS} meets the margin")
        mg = min(margin(a32), margin(a64))
        assert mg >= T.MARGIN and same_masks(a32, a64)
        print(f"{name}: seed {seed} (walked {seed - SEED0}), margin {mg:.3e}", flush=True)
        out[f"{name}/seed"], out[f"{name}/margin"] = np.int64(seed), np.float64(mg)
        for s, (r32, r64) in enumerate(zip(s32, s64), start=1):
            out[f"{name}/loss{s}"] = np.float64(r32['loss'])
            out[f"{name}_d64/loss{s}"] = np.float64(r64['loss'] - r32['loss'])
            for kind in ('g', 'w', 'b'):
                for k, v32 in r32[kind].items():
                    if not v32.is_floating_point():
                        assert torch.equal(v32, r64[kind][k])
                        out[f"{name}/{kind}{s}/{k}"] = v32.numpy()
                        continue
                    d = r64[kind][k] - v32.double()
                    out[f"{name}/{kind}{s}/{k}"] = T.sample(v32.numpy()).astype(np.float32)
                    out[f"{name}_d64/{kind}{s}/{k}"] = T.sample(d.numpy()).astype(np.float32)
                    out[f"{name}/gap_{kind}{s}/{k}"] = np.float64(d.abs().max())
                    if kind == 'g':
                        out[f"{name}/gmax{s}/{k}"] = np.float64(v32.abs().max())
            for i, a in a32[s - 1].items():
                out[f"{name}/mask{s}/{i}"] = np.packbits((a > 0).permute(0, 2, 3, 1).contiguous().numpy().reshape(-1))
            print(f"  step {s}: loss {r32['loss']:.8f} (float64 {r64['loss'] - r32['loss']:+.2e}), worst gradient gap "
                  f"{max(float(out[f'{name}/gap_g{s}/{k}']) / max(float(out[f'{name}/gmax{s}/{k}']), 1e-30) for k in r32['g']):.2e} of its tensor's largest",
                  flush=True)
        out[f"{name}/eval"] = y32.numpy().astype(np.float32)
        out[f"{name}_d64/eval"] = (y64 - y32.double()).numpy().astype(np.float32)
    save_npz(OUT, out)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
