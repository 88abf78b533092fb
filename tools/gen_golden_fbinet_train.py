"""TEST INFRASTRUCTURE ONLY -- write tests/golden/fbinet_train.npz by running the reference trainer's own step on its FBI_Net, on CPU.

Run where the reference tree exists (not on the GPU box):

    python tools/gen_golden_fbinet_train.py

It imports the reference under the stub modules of `oracle/_refimport.py` (used as is), with `.cuda()` neutralised as in
tools/gen_golden_fbinet.py, and stores RESULTS and seeds only; weights and batches are regenerated from the seed by
tests/fbinet_train_common.py.  Per case (fbinet_train_common.CASES: nf 32, 3 layers, one 8 x 12 mosaic; `lin`: res with 2 outputs,
linear; `sig`: the same with output_type sigmoid; `nores`: res off, 1 output, Charbonnier loss) the reference's FBI_Net
(archs/comp.py:264-648) takes two consecutive steps of trainer_AWGN.py:85-117 -- net.train(); optimizer.zero_grad(); pred = net(lr);
loss = Unet_Loss(charbonnier)(pred, hr); loss.backward(); Adam(net.parameters(), lr).step() -- once in float32 and once in float64.
Stored per step s = 1, 2 (one array per step and kind: fbinet_train_common.flat puts the tensors' samples back to back in the order of
<c>/params, the reference's named_parameters()):
    <c>/loss<s>        the float32 loss (as float64)          <c>_d64/...: the float64 run minus the float32 one
    <c>/g<s>           every gradient ON THE LIVE TAPS (dead taps set to zero), sampled;  <c>_d64/g<s>: float64 minus float32, alike
    <c>/w<s>           every updated parameter, alike, float32 run only (the reference's Adam moves its dead taps; its next forward
                       zeroes them)
    <c>/stat<s>        per parameter: max |float32 - float64| of the gradient and of the weight, max |gradient|, each over the WHOLE
                       tensor's live taps (gap_g, gap_w, gmax)
    <c>/mask<s>        the branch (input > 0) of every PReLU in forward order (fbinet_train_common.prelu_names), [N][H][W][C] each, np.packbits
and <c>/seed, <c>/margin.

Condition on the inputs: a PReLU's derivative is discontinuous at zero.  Seeds are walked from SEED0 until, in both steps, the float32
and the float64 run take the same branch at every PReLU and no PReLU input lies within 1e-5 of its layer's RMS of zero
(fbinet_train_common.MARGIN: of this shape's 43,008 inputs 5-9 lie under 1e-4, so that margin would not end the walk)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import _refimport  # noqa: E402
import fbinet_train_common as T  # noqa: E402
from gen_golden_estnet import save_npz  # noqa: E402
from gen_golden_fbinet import REF_KEYS  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "fbinet_train.npz")
SEED0 = 20261023
MAX_SEEDS = 100000


def run(ref, name, seed, dtype):
    """Two steps.  Returns (records per step, PReLU inputs per step {slope name: tensor})."""
    args, charb = T.CASES[name]
    net = ref.FBI_Net({k: args[k] for k in REF_KEYS})
    sd = {k: torch.as_tensor(v).clone() for k, v in T.weights(name, seed).items()}
    ref.load_weights(net, sd, by_name=False)
    net = net.to(dtype)
    for m in net.modules():                                   # (the masks are plain attributes: .to() does not reach them)
        if hasattr(m, 'mask'):
            m.mask = m.mask.to(dtype)
    pres = {}
    for n, m in net.named_modules():
        if isinstance(m, torch.nn.PReLU):
            m.register_forward_pre_hook(lambda mod, inp, n=n: pres.__setitem__(n + '.weight', inp[0].detach().clone()))
    loss_fn = ref.Unet_Loss(charbonnier=charb)
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
        steps.append(dict(loss=float(loss.detach()), g=grads, w={n: p.detach().clone() for n, p in net.named_parameters()}))
    assert list(acts[0]) == T.prelu_names(args), list(acts[0])
    return steps, acts


def margin(acts):
    return min(float(a.abs().min() / a.double().pow(2).mean().sqrt()) for step in acts for a in step.values())


def same_masks(a32, a64):
    return all(torch.equal(s32[i] > 0, s64[i] > 0) for s32, s64 in zip(a32, a64) for i in s32)


def main():
    torch.set_num_threads(8)
    ref = _refimport.import_reference()
    torch.nn.Module.cuda = lambda self, *a, **k: self
    torch.Tensor.cuda = lambda self, *a, **k: self
    out = {}
    for name in T.CASES:
        for seed in range(SEED0, SEED0 + MAX_SEEDS):
            s32, a32 = run(ref, name, seed, torch.float32)
            if margin(a32) < T.MARGIN:
                continue
            s64, a64 = run(ref, name, seed, torch.float64)
            if margin(a64) >= T.MARGIN and same_masks(a32, a64):
                break
        else:
            raise SystemExit(f"{name}: no seed in {MAX_SEEDS} meets the margin")
        mg = min(margin(a32), margin(a64))
        print(f"{name}: seed {seed} (walked {seed - SEED0}), margin {mg:.3e}", flush=True)
        out[f"{name}/seed"], out[f"{name}/margin"] = np.int64(seed), np.float64(mg)
        for s, (r32, r64) in enumerate(zip(s32, s64), start=1):
            out[f"{name}/loss{s}"] = np.float64(r32['loss'])
            out[f"{name}_d64/loss{s}"] = np.float64(r64['loss'] - r32['loss'])
            names = list(r32['g'])
            g32, g64 = ({k: v.double().numpy() for k, v in r['g'].items()} for r in (r32, r64))
            w32, w64 = ({k: v.double().numpy() for k, v in r['w'].items()} for r in (r32, r64))
            out[f"{name}/params"] = np.array(names)
            out[f"{name}/g{s}"] = T.flat(g32, names)[0].astype(np.float32)
            out[f"{name}_d64/g{s}"] = T.flat({k: g64[k] - g32[k] for k in names}, names)[0].astype(np.float32)
            out[f"{name}/w{s}"] = T.flat(w32, names)[0].astype(np.float32)
            live = {k: T.live_mask(k, g32[k].shape) for k in names}
            out[f"{name}/stat{s}"] = np.array([[np.abs((g64[k] - g32[k]) * live[k]).max(), np.abs((w64[k] - w32[k]) * live[k]).max(),
                                                 np.abs(g32[k] * live[k]).max()] for k in names], np.float64)
            out[f"{name}/mask{s}"] = T.mask_bits({k: v.permute(0, 2, 3, 1).numpy() for k, v in a32[s - 1].items()}, T.prelu_names(T.CASES[name][0]))
            print(f"  step {s}: loss {r32['loss']:.8f} (float64 {r64['loss'] - r32['loss']:+.2e}), worst gradient gap "
                  f"{float((out[f'{name}/stat{s}'][:, 0] / np.maximum(out[f'{name}/stat{s}'][:, 2], 1e-30)).max()):.2e} of its tensor's largest",
                  flush=True)
    save_npz(OUT, out)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
