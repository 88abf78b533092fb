"""GPU: training FBI_Net on the HIP kernels (yond_public_amd/train.py: TrainStep._forward_fbi over csrc/fbinet.hip and
csrc/fbinet_train.hip) against two steps of the reference trainer (tests/golden/fbinet_train.npz, tools/gen_golden_fbinet_train.py),
against the float64 model with the HIP forward's PReLU branches forced (tests/fbinet_train_model.py), the captured step against the
eager one, the dead taps, the training forward against the module's own, and the trainer_AWGN driver on
runfiles/Gaussian/FBI_5to50_norm.yml.

Tolerances of the golden parity are those of tests/test_hip_dncnn_train.py: loss max(2e-5 rel, 8 gaps); per tensor, gradients
max(5e-4 of the tensor's largest gradient, 8 times the reference's own |float32 - float64| gap); updated weights by the counting rule
(Adam moves every weight by about lr per step whatever its gradient's size, so only weights whose gradient is within its tolerance of
zero may land elsewhere: at most 2e-3 of them per step beyond max(2e-3 lr per step, 8 gaps)).  Parity is on the live taps: the
reference's dense autograd moves its dead taps, which its next forward zeroes again; here their gradient is zero and they stay untouched.
The measured error / limit ratios go into profiles/fbinet_train_report.txt (YOND_FBI_REPORT=<file> appends the [parity] lines there)."""
import os

import numpy as np
import pytest
import torch

import fbinet_common as D
import fbinet_train_common as T
import fbinet_train_model as M

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def note(line):
    print(line)
    path = os.environ.get("YOND_FBI_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def make(args, sd):
    from yond_public_amd import archs as A
    net = A.FBI_Net(dict(args))
    net.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return net.to(DEV).train()


def packed(mosaic):
    """[N][1][H][W] -> the trainer's packed batch [N][4][h][w]."""
    return D.to_packed(mosaic).permute(0, 3, 1, 2).contiguous().to(DEV)


@pytest.mark.parametrize("name", ["lin", "sig", "nores"])
def test_two_steps_match_the_reference_trainer(golden, name):
    from yond_public_amd.train import TrainStep
    g = golden("fbinet_train")
    args, charb = T.CASES[name]
    seed = int(g[f"{name}/seed"])
    names = [str(k) for k in g[f"{name}/params"]]
    sd0 = T.weights(name, seed)
    net = make(args, sd0)
    ts = TrainStep(net, lr=T.LR, charbonnier=charb, graph=False)
    assert list(ts.params) == names and ts.plan.train_conv == 'fp32'
    ts.keep_acts = True
    for s in (1, 2):
        lr_img, hr_img = T.batch(seed, s - 1)
        loss, grads = ts.step(packed(lr_img), packed(hr_img))
        torch.cuda.synchronize()
        assert ts.last_scale == 1.0 and list(ts.last_acts) == T.prelu_names(args)
        own = T.mask_bits({k: v.cpu().numpy() for k, v in ts.last_acts.items()}, T.prelu_names(args))
        flipped = int(np.unpackbits(own ^ g[f"{name}/mask{s}"]).sum())
        ref_loss, gap_loss = float(g[f"{name}/loss{s}"]), abs(float(g[f"{name}_d64/loss{s}"]))
        lim = max(2e-5 * abs(ref_loss), 8 * gap_loss)
        note(f"[parity] fbinet_train {name} step {s}: loss {loss:.9f} vs {ref_loss:.9f}: |diff| {abs(loss - ref_loss):.2e}  limits 2e-5 rel "
             f"{2e-5 * abs(ref_loss):.2e}, 8 gaps {8 * gap_loss:.2e}; {flipped} of {own.size * 8} PReLU inputs on the other branch than the reference's")
        assert abs(loss - ref_loss) <= lim
        got, segs = T.flat({k: v.cpu().numpy() for k, v in grads.items()}, names)
        ref, stat = g[f"{name}/g{s}"].astype(np.float64), g[f"{name}/stat{s}"]
        worst = ("", 0.0)
        for (k, a, b), (gap_g, gap_w, gmax) in zip(segs, stat):
            err, lim = float(np.abs(got[a:b] - ref[a:b]).max()), max(5e-4 * gmax, 8 * gap_g)
            if err / lim > worst[1]:
                worst = (k, err / lim)
            assert err <= lim, (s, k, err, 5e-4 * gmax, 8 * gap_g)
        gotw, _ = T.flat({k: p.detach().cpu().numpy() for k, p in ts.params.items()}, names)
        refw = g[f"{name}/w{s}"].astype(np.float64)
        bad = sum(int((np.abs(gotw[a:b] - refw[a:b]) > max(2e-3 * T.LR * s, 8 * gap_w)).sum()) for (k, a, b), (_, gap_w, _) in zip(segs, stat))
        note(f"[parity] fbinet_train {name} step {s}: worst gradient error / limit {worst[1]:.3f} ({worst[0]}); {bad} of {gotw.size} stored weights "
             f"beyond max(2e-3 lr per step, 8 gaps), allowed {int(2e-3 * s * gotw.size)}")
        assert bad <= 2e-3 * s * gotw.size
    # dead taps: no gradient, bit for bit the values the module was built with
    for k, p in ts.params.items():
        dead = torch.from_numpy(np.ascontiguousarray(T.live_mask(k, tuple(p.shape)) == 0))
        if bool(dead.any()):
            assert torch.equal(p.detach().cpu()[dead], torch.as_tensor(sd0[k])[dead]), k
            assert float(grads[k].cpu()[dead].abs().max()) == 0.0, k
            assert not torch.equal(p.detach().cpu()[~dead], torch.as_tensor(sd0[k])[~dead]), k


@pytest.mark.parametrize("name", ["a", "e"])
def test_gradients_match_the_float64_model_on_the_forwards_own_branches(golden, name):
    """fbinet_common.CASES a (2 x 24 x 40, nf 32) and e (3 x 38 x 50, nf 64), L 4, procedural weights: every gradient against the float64
    model run with each PReLU's branch forced to the HIP forward's, at 5e-4 of the tensor's largest gradient.  The forced branch must be
    the model's own wherever the model's |input| is at least 1e-4 of its layer's RMS, and at most 5e-4 of the inputs may lie under that
    margin (the float64 model alone: 1.0e-4 to 2.1e-4 on these cases)."""
    from yond_public_amd.train import TrainStep
    g = golden("fbinet")
    args, shape = D.CASES[name]
    sd = D.weights(args, D.case_seed(g["w_seed"], name))
    x, tgt = D.case_input(shape, D.case_seed(g["x_seed"], name)), D.case_input(shape, 99)
    ts = TrainStep(make(args, sd), lr=1e-3, graph=False)
    ts.keep_acts = True
    loss, grads = ts.step(packed(x), packed(tgt))
    torch.cuda.synchronize()
    forced = {k: (v > 0).permute(0, 3, 1, 2).cpu() for k, v in ts.last_acts.items()}
    _, _, own, _ = M.grads64(args, sd, x, tgt, False)
    under = total = 0
    for k, v in own.items():
        rms = float(v.pow(2).mean().sqrt())
        safe = v.abs() >= 1e-4 * rms
        assert torch.equal(forced[k][safe], (v > 0)[safe]), k
        under += int((~safe).sum())
        total += v.numel()
    mloss, mgrads, _, _ = M.grads64(args, sd, x, tgt, False, masks=forced)
    worst = ("", 0.0)
    for k, mg in mgrads.items():
        gmax = float(mg.abs().max())
        err = float((grads[k].cpu().double() - mg).abs().max())
        if err / (5e-4 * gmax) > worst[1]:
            worst = (k, err / (5e-4 * gmax))
        assert err <= 5e-4 * gmax, (k, err, gmax)
    note(f"[parity] fbinet_train forced branches ({name}): loss {loss:.9f} vs model {mloss:.9f}; worst gradient error / (5e-4 of largest) "
         f"{worst[1]:.4f} ({worst[0]}); {under} of {total} PReLU inputs under 1e-4 RMS ({under / total:.2e}, allowed 5e-4)")
    assert abs(loss - mloss) <= 2e-5 * abs(mloss)
    assert under <= 5e-4 * total


def _batches(n, seed, shape=(2, 1, 16, 24)):
    out = []
    for k in range(n):
        g = torch.Generator().manual_seed(seed * 16 + k)
        hr = torch.rand(shape, generator=g) * 0.8 + 0.05
        out.append((packed((hr + torch.randn(shape, generator=g) * 0.08).clamp(0, 1)), packed(hr)))
    return out


def test_graph_replayed_steps_match_eager_steps():
    """Five steps with changing batches: from the third on the step replays as one hipGraph.  The rule of the existing graph tests:
    losses to rtol 1e-6, tensors to 1e-4.  Every reduction of this arch has a fixed order, so the bits are expected to agree too
    (printed); two eager runs from the same start ARE asserted bit-equal."""
    from yond_public_amd.train import TrainStep
    args = D.fbi_args(nf=32, num_of_layers=4, output_type='sigmoid')
    sd = D.weights(args, 5)
    batches = _batches(5, 77)
    out = {}
    for tag, graph in (("eager", False), ("eager2", False), ("graph", True)):
        net = make(args, sd)
        ts = TrainStep(net, lr=1e-3, graph=graph)
        losses = [ts.step(a, b)[0] for a, b in batches]
        torch.cuda.synchronize()
        assert bool(ts._graphs) == graph and ts.t == 5
        out[tag] = (losses, {k: p.detach().clone() for k, p in net.named_parameters()})
    (le, we), (l2, w2), (lg, wg) = out["eager"], out["eager2"], out["graph"]
    assert le == l2 and all(torch.equal(we[k].view(torch.int32), w2[k].view(torch.int32)) for k in we)
    assert np.allclose(le, lg, rtol=1e-6, atol=0), (le, lg)
    for k in we:
        assert float((we[k] - wg[k]).abs().max()) <= 1e-4, k
    assert any(not torch.equal(we[k], torch.as_tensor(sd[k]).to(DEV)) for k in we)
    same = all(torch.equal(we[k], wg[k]) for k in we)
    print(f"[parity] fbinet_train graph vs eager: losses {le} / {lg}; weights bitwise equal: {same}")


@pytest.mark.parametrize("name", ["a", "e"])
def test_training_forward_equals_the_inference_forward(golden, name):
    """TrainStep.forward (unfused launches) against net(x) (the fused inference kernels) on the same weights: the bound
    tests/test_hip_fbinet.py holds the forward to, 1e-4 max(1, max |ref|)."""
    from yond_public_amd.train import TrainStep
    g = golden("fbinet")
    args, shape = D.CASES[name]
    net = make(args, D.weights(args, D.case_seed(g["w_seed"], name)))
    x = D.case_input(shape, D.case_seed(g["x_seed"], name))
    ts = TrainStep(net, graph=False)
    with torch.no_grad():
        ts._gather_weights()
        y_train = D.from_packed(ts.forward(packed(x)).permute(0, 2, 3, 1).contiguous()).cpu().numpy()
        y = net.eval()(x.to(DEV)).cpu().numpy()
    err = float(np.abs(y_train - y).max())
    print(f"[parity] fbinet_train forward ({name}): max |training forward - net(x)| {err:.2e}")
    assert err <= 1e-4 * max(1.0, float(np.abs(y).max()))
    ref = g[f"y32_{name}"]
    assert float(np.abs(y_train - ref).max()) <= 1e-4 * max(1.0, float(np.abs(ref).max()))


def _small_runfile(tmp_path, **hyper_over):
    import yaml
    cfg = yaml.load(open(os.path.join(ROOT, "runfiles", "Gaussian", "FBI_5to50_norm.yml")).read(), Loader=yaml.FullLoader)
    plug = yaml.load(open(os.path.join(ROOT, "runfiles", "YOND", "ANY_simple+full_pre_fbi.yml")).read(), Loader=yaml.FullLoader)
    assert cfg["arch"] == plug["arch"] and cfg["model_name"] == plug["model_name"] and cfg["fast_ckpt"] == plug["fast_ckpt"]
    cfg["arch"].update(nf=32, num_of_layers=3)
    for sec in ("dst", "dst_train", "dst_eval", "dst_test"):
        cfg[sec].update(H=32, W=32, patch_size=32, root_dir=str(tmp_path / "nodata"), dataset='RGB_Img2Raw_Dataset')
    cfg["hyper"].update(batch_size=4, last_epoch=0, stop_epoch=3, step_size=1, T=1, coldstart=True, save_freq=1, plot_freq=1, learning_rate=1e-3)
    cfg["hyper"].update(hyper_over)
    rf = tmp_path / f"small_fbi_{cfg['hyper']['last_epoch']}_{cfg['hyper']['stop_epoch']}.yml"
    rf.write_text(yaml.dump(cfg))
    return str(rf), cfg, plug


def test_trainer_awgn_driver_trains_evaluates_saves_and_resumes(tmp_path, monkeypatch, golden):
    from yond_public_amd import archs as A
    from yond_public_amd import trainer_AWGN as TA
    monkeypatch.chdir(tmp_path)
    argv = lambda rf, epochs: ['-f', rf, '-m', 'train', '--synthetic', '8', '--epochs', str(epochs)]
    torch.manual_seed(3)
    rf, cfg, plug = _small_runfile(tmp_path)
    out = TA.main(argv(rf, 2))
    hist = out['history']
    assert [h[0] for h in hist] == [1, 2] and all(len(h[2]) == 2 and np.isfinite(h[2]).all() for h in hist)
    assert np.isfinite(out['psnr_sig25']) and out['psnr_sig25'] > 5
    name = cfg['model_name']
    for f in (f"checkpoints/Gaussian/{name}_last_model.pth", f"saved_model/Gaussian/{name}_e0002.pth", f"logs/log_{name}.log"):
        assert os.path.exists(f), f
    sd = torch.load(f"checkpoints/Gaussian/{name}_last_model.pth", map_location='cpu')
    # the reference's keys, shapes and order: those of fixture case (a) but for the layer count (a has one more dilated layer, new_1)
    want = [str(k)[2:] for k in golden("fbinet")["keys"] if str(k).startswith("a:") and not str(k).startswith("a:new_1.")]
    assert [f"{k}:{'x'.join(map(str, v.shape))}" for k, v in sd.items()] == want
    # interrupted after epoch 1 and resumed from its checkpoint: epoch 2 starts from the same weights
    for f in os.listdir("checkpoints/Gaussian"):
        os.remove(os.path.join("checkpoints/Gaussian", f))
    torch.manual_seed(3)
    h1 = TA.main(argv(rf, 1))['history']
    assert np.allclose(h1[0][2], hist[0][2], rtol=1e-6, atol=0)
    rf2, _, _ = _small_runfile(tmp_path, last_epoch=1)
    tr = TA.AWGN_Trainer(argv(rf2, 1))
    h2 = tr.train()
    assert [h[0] for h in h2] == [2]
    # (the reference's checkpoints hold no optimiser state: only the FIRST loss of the resumed epoch is the uninterrupted run's)
    assert np.isclose(h2[0][2][0], hist[1][2][0], rtol=1e-6, atol=0), (h2, hist)
    # the checkpoint loads strictly into the plug-in the YOND runfile names, whose forward is the trained module's
    sd2 = torch.load(f"{plug['fast_ckpt']}/{plug['model_name']}_last_model.pth", map_location='cpu')
    fresh = A.FBI_Net(dict(plug['arch'], nf=32, num_of_layers=3))
    TA.load_weights(fresh, sd2, by_name=False)
    res = fresh.load_state_dict(sd2, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    fresh = fresh.to(DEV).eval()
    x = D.case_input((1, 1, 32, 32), 4).to(DEV)
    assert torch.equal(fresh(x), tr.net.eval()(x))


def test_a_process_group_is_refused(tmp_path):
    import torch.distributed as dist
    from yond_public_amd import _lib as L
    from yond_public_amd.train import TrainStep
    args = D.fbi_args(nf=32, num_of_layers=3)
    assert not dist.is_initialized()
    dist.init_process_group('gloo', init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        with pytest.raises(L.YondHipError, match="process group"):
            TrainStep(make(args, D.weights(args, 1)), ddp=None)
        TrainStep(make(args, D.weights(args, 1)), ddp=False)
    finally:
        dist.destroy_process_group()


def test_a_batch_that_is_not_packed_is_refused_before_any_launch():
    """The step takes the trainer's packed [N][4][h][w] batches: the one-channel mosaic the module's own forward takes is refused by
    name, with nothing launched and no parameter touched."""
    from yond_public_amd.train import TrainStep
    args = D.fbi_args(nf=32, num_of_layers=3)
    sd = D.weights(args, 2)
    net = make(args, sd)
    ts = TrainStep(net, graph=False)
    x = torch.rand((1, 1, 16, 16), device=DEV)
    with pytest.raises(NotImplementedError, match="FBI_Net"):
        ts.step(x, x)
    assert ts.t == 0 and all(torch.equal(p.detach().cpu(), torch.as_tensor(sd[k])) for k, p in net.named_parameters())
