"""GPU: training DnCNN on the HIP kernels (yond_public_amd/train.py: TrainStep._forward_dncnn, _BatchNormRelu over csrc/bn_train.hip)
against the reference trainer's own steps (tests/golden/dncnn_train.npz, tools/gen_golden_dncnn_train.py), the captured step against
the eager one, the redo path's running statistics, the trainer_AWGN driver on runfiles/Gaussian/DnCNN_5to50_norm.yml, and what
stays refused.

Tolerances of the golden parity, per tensor: the larger of (a) the project's training tolerance -- 5e-4 of the tensor's largest gradient,
rtol 2e-5 on the loss (tests/test_hip_train.py) -- and (b) eight times the reference's own |float32 - float64| gap for that tensor, stored
in the fixture (8: the split-operand products carry 22-bit operands against float32's 24).  Buffers are forward quantities and take the
loss's 2e-5 (of the tensor's largest value) for (a).  Updated parameters take the existing tests' counting rule: Adam moves every weight by
about +-lr per step, so only weights whose gradient is within its tolerance of zero may land elsewhere -- at most 2e-3 of them per step
may be off by more than max(2e-3 lr per step, 8 gaps).  The measured errors go beside both limits into profiles/bn_train_report.txt
(YOND_BN_REPORT=<file> appends the [parity] lines there)."""
import os

import numpy as np
import pytest
import torch

import dncnn_train_common as T
from test_hip_bn_train import note

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make(name, seed):
    from yond_public_amd import archs as A
    net = A.DnCNN(dict(T.VARIANTS[name]))
    net.load_state_dict({k: torch.as_tensor(v) for k, v in T.weights(name, seed).items()})
    return net.to(DEV).train()


@pytest.mark.parametrize("conv", ["split", "fp32"])
@pytest.mark.parametrize("name", ["bn", "nobn"])
def test_two_steps_match_the_reference_trainer(golden, name, conv):
    from yond_public_amd.train import TrainStep
    g = golden("dncnn_train")
    seed = int(g[f"{name}/seed"])
    net = make(name, seed)
    ts = TrainStep(net, lr=T.LR, conv=conv, graph=False)
    ts.keep_acts = True
    for s in (1, 2):
        lr_img, hr_img = T.batch(seed, s - 1)
        loss, grads = ts.step(lr_img.to(DEV), hr_img.to(DEV))
        torch.cuda.synchronize()
        # the ReLU masks first: a flipped pre-activation makes the gradients incomparable, and is reported as that
        for i in T.relu_indices(name):
            own = np.packbits((ts.last_acts[i] > 0).cpu().numpy().reshape(-1))
            flipped = int(np.unpackbits(own ^ g[f"{name}/mask{s}/{i}"]).sum())
            if flipped:
                pytest.fail(f"ReLU MASK MISMATCH (not a gradient error): step {s}, dncnn.{i}: {flipped} of {own.size * 8} pre-activations "
                            f"have another sign than in the reference's float32 run")
        ref_loss, gap_loss = float(g[f"{name}/loss{s}"]), abs(float(g[f"{name}_d64/loss{s}"]))
        lim = max(2e-5 * abs(ref_loss), 8 * gap_loss)
        note(f"[parity] dncnn_train {name} {conv} step {s}: loss {loss:.9f} vs {ref_loss:.9f}: |diff| {abs(loss - ref_loss):.2e}  "
             f"limits 2e-5 rel {2e-5 * abs(ref_loss):.2e}, 8 gaps {8 * gap_loss:.2e}")
        assert abs(loss - ref_loss) <= lim
        worst = ("", 0.0)
        for k in ts.params:
            ref = g[f"{name}/g{s}/{k}"]
            err = float(np.abs(T.sample(grads[k].cpu().numpy()).astype(np.float64) - ref).max())
            lim_a, lim_b = 5e-4 * float(g[f"{name}/gmax{s}/{k}"]), 8 * float(g[f"{name}/gap_g{s}/{k}"])
            note(f"[parity] dncnn_train {name} {conv} step {s}: gradient {k}: max |diff| {err:.2e}  limits 5e-4 of largest {lim_a:.2e}, 8 gaps {lim_b:.2e}")
            if err / max(lim_a, lim_b) > worst[1]:
                worst = (k, err / max(lim_a, lim_b))
            assert err <= max(lim_a, lim_b), (k, err, lim_a, lim_b)
        bad, n = 0, 0
        for k, p in ts.params.items():
            ref = g[f"{name}/w{s}/{k}"]
            dw = np.abs(T.sample(p.detach().cpu().numpy()).astype(np.float64) - ref)
            thr = max(2e-3 * T.LR * s, 8 * float(g[f"{name}/gap_w{s}/{k}"]))
            bad += int((dw > thr).sum())
            n += dw.size
        note(f"[parity] dncnn_train {name} {conv} step {s}: worst gradient error / limit {worst[1]:.3f} ({worst[0]}); {bad} of {n} stored weights "
             f"beyond max(2e-3 lr per step, 8 gaps), allowed {int(2e-3 * s * n)}")
        assert bad <= 2e-3 * s * n
        for k, b in net.named_buffers():
            ref = g[f"{name}/b{s}/{k}"]
            if k.endswith('num_batches_tracked'):
                assert int(b) == int(ref) == s, k
                continue
            err = float(np.abs(b.cpu().numpy().astype(np.float64) - ref).max())
            lim_a, lim_b = 2e-5 * float(np.abs(ref).max()), 8 * float(g[f"{name}/gap_b{s}/{k}"])
            note(f"[parity] dncnn_train {name} {conv} step {s}: buffer {k}: max |diff| {err:.2e}  limits 2e-5 of largest {lim_a:.2e}, 8 gaps {lim_b:.2e}")
            assert err <= max(lim_a, lim_b), (k, err, lim_a, lim_b)
    # plan invalidation: the inference plan must fold the statistics the two steps left (tests/test_hip_dncnn.py's float32 bound)
    x3 = T.batch(seed, 2)[0].to(DEV)
    if T.VARIANTS[name]['use_bn']:
        with pytest.raises(Exception, match="train"):         # (the module's own forward stays inference only)
            net(x3)
    y = net.eval()(x3).cpu().numpy()
    ref = g[f"{name}/eval"]
    err = float(np.abs(y - ref).max())
    note(f"[parity] dncnn_train {name} {conv}: eval-mode output after step 2: max |diff| {err:.2e}  limit {1e-4 * max(1.0, float(np.abs(ref).max())):.2e}")
    assert err <= 1e-4 * max(1.0, float(np.abs(ref).max()))


def _batches(n, seed):
    return [tuple(t.to(DEV) for t in T.batch(seed, k)) for k in range(n)]


def test_graph_replayed_steps_match_eager_steps():
    """Five steps with changing batches: from the third on the step (BatchNorm launches included) replays as one hipGraph; the
    running statistics are committed behind each replay's verdict.  The rule of tests/test_hip_train.py's graph test: losses to rtol
    1e-6, tensors to 1e-4 (the first layer's bias gradient comes from float atomics: last-bit differences), counters equal."""
    from yond_public_amd.train import TrainStep
    batches = _batches(5, 77)
    out = {}
    for graph in (False, True):
        net = make('bn', 5)
        ts = TrainStep(net, lr=1e-3, graph=graph)
        losses = [ts.step(lr_img, hr_img)[0] for lr_img, hr_img in batches]
        torch.cuda.synchronize()
        assert bool(ts._graphs) == graph and ts.t == 5
        out[graph] = (losses, {k: b.detach().clone() for k, b in net.named_buffers()}, {k: p.detach().clone() for k, p in net.named_parameters()})
    (le, be, we), (lg, bg, wg) = out[False], out[True]
    assert np.allclose(le, lg, rtol=1e-6, atol=0), (le, lg)
    for k in be:
        if k.endswith('num_batches_tracked'):
            assert int(be[k]) == int(bg[k]) == 5
        else:
            assert float((be[k] - bg[k]).abs().max()) <= 1e-4, k
    for k in we:
        assert float((we[k] - wg[k]).abs().max()) <= 1e-4, k
    same = all(torch.equal(be[k], bg[k]) for k in be)
    print(f"[parity] dncnn_train graph vs eager: losses {le} / {lg}; buffers bitwise equal: {same}")


def test_a_redone_step_advances_the_running_statistics_once():
    """loss_scale 2^20: dpred = 512 trips the weight gradient's range guard, the step is redone at 2^12.  The forward does not depend on
    the scale: buffers bitwise equal to those of a run at the automatic scale, one batch tracked."""
    from yond_public_amd.train import TrainStep
    (lr_img, hr_img), = _batches(1, 78)
    bufs = {}
    for scale in (None, 2.0 ** 20):
        net = make('bn', 6)
        ts = TrainStep(net, lr=1e-3, loss_scale=scale, graph=False)
        loss, _ = ts.step(lr_img, hr_img)
        torch.cuda.synchronize()
        assert np.isfinite(loss)
        if scale is not None:
            assert ts.last_scale < scale                      # the first attempt overflowed
        bufs[scale] = {k: b.detach().cpu().clone() for k, b in net.named_buffers()}
    for k, a in bufs[None].items():
        b = bufs[2.0 ** 20][k]
        if k.endswith('num_batches_tracked'):
            assert int(a) == int(b) == 1
        else:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k
            assert not torch.equal(a, torch.as_tensor(T.weights('bn', 6)[k]))          # (they did move)


def _small_runfile(tmp_path, **hyper_over):
    import yaml
    cfg = yaml.load(open(os.path.join(ROOT, "runfiles", "Gaussian", "DnCNN_5to50_norm.yml")).read(), Loader=yaml.FullLoader)
    assert cfg["arch"] == dict(name='DnCNN', in_nc=4, out_nc=4, nf=64, depth=17, use_bn=True, res=True)
    cfg["arch"].update(nf=32, depth=4)
    for sec in ("dst", "dst_train", "dst_eval", "dst_test"):
        cfg[sec].update(H=32, W=32, patch_size=32, root_dir=str(tmp_path / "nodata"), dataset='RGB_Img2Raw_Dataset')
    cfg["hyper"].update(batch_size=4, last_epoch=0, stop_epoch=3, step_size=1, T=1, coldstart=True, save_freq=1, plot_freq=1, learning_rate=1e-3)
    cfg["hyper"].update(hyper_over)
    rf = tmp_path / f"small_dncnn_{cfg['hyper']['last_epoch']}_{cfg['hyper']['stop_epoch']}.yml"
    rf.write_text(yaml.dump(cfg))
    return str(rf), cfg


def test_trainer_awgn_driver_trains_evaluates_saves_and_resumes(tmp_path, monkeypatch, golden):
    from yond_public_amd import archs as A
    from yond_public_amd import trainer_AWGN as TA
    monkeypatch.chdir(tmp_path)
    argv = lambda rf, epochs: ['-f', rf, '-m', 'train', '--synthetic', '8', '--epochs', str(epochs)]
    # an uninterrupted run of two epochs (2 batches each) of the schedule's three, an evaluation behind each
    torch.manual_seed(3)
    rf, cfg = _small_runfile(tmp_path)
    out = TA.main(argv(rf, 2))
    hist = out['history']
    assert [h[0] for h in hist] == [1, 2] and all(len(h[2]) == 2 and np.isfinite(h[2]).all() for h in hist)
    assert np.isfinite(out['psnr_sig25']) and out['psnr_sig25'] > 5
    name = cfg['model_name']
    for f in (f"checkpoints/Gaussian/{name}_last_model.pth", f"saved_model/Gaussian/{name}_e0002.pth", f"logs/log_{name}.log"):
        assert os.path.exists(f), f
    sd = torch.load(f"checkpoints/Gaussian/{name}_last_model.pth", map_location='cpu')
    want = [str(k)[2:] for k in golden("dncnn")["keys"] if str(k).startswith("a:")]          # the reference's keys and shapes (nf 32, depth 4)
    assert [f"{k}:{'x'.join(map(str, v.shape))}" for k, v in sd.items()] == want
    assert all(int(v) == 4 for k, v in sd.items() if k.endswith('num_batches_tracked'))
    # the same, interrupted after epoch 1 and resumed from its checkpoint: epoch 2 starts from the same weights and statistics
    for f in os.listdir("checkpoints/Gaussian"):
        os.remove(os.path.join("checkpoints/Gaussian", f))
    torch.manual_seed(3)
    h1 = TA.main(argv(rf, 1))['history']
    assert np.allclose(h1[0][2], hist[0][2], rtol=1e-6, atol=0)
    rf2, _ = _small_runfile(tmp_path, last_epoch=1)
    tr = TA.AWGN_Trainer(argv(rf2, 1))
    assert all(int(b) == 2 for k, b in tr.net.named_buffers() if k.endswith('num_batches_tracked'))
    h2 = tr.train()
    assert [h[0] for h in h2] == [2]
    # (the reference's checkpoints hold no optimiser state: Adam's moments restart, so only the FIRST loss of the resumed epoch -- taken before
    #  any update -- is the uninterrupted run's)
    assert np.isclose(h2[0][2][0], hist[1][2][0], rtol=1e-6, atol=0), (h2, hist)
    # the checkpoint loads strictly into the inference plug-in, whose forward is the trained module's eval forward bit for bit
    sd2 = torch.load(f"checkpoints/Gaussian/{name}_last_model.pth", map_location='cpu')
    fresh = A.DnCNN(dict(cfg['arch']))
    TA.load_weights(fresh, sd2, by_name=False)
    res = fresh.load_state_dict(sd2, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    fresh = fresh.to(DEV).eval()
    x = T.batch(9, 2)[0].to(DEV)
    assert torch.equal(fresh(x), tr.net.eval()(x))


def test_batchnorm_under_a_process_group_is_refused(tmp_path):
    import torch.distributed as dist
    from yond_public_amd import _lib as L
    from yond_public_amd.train import TrainStep
    assert not dist.is_initialized()
    dist.init_process_group('gloo', init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        with pytest.raises(L.YondHipError, match="process group"):
            TrainStep(make('bn', 1), ddp=None)
        TrainStep(make('bn', 1), ddp=False)                   # (no exchange asked for: one process's own statistics)
    finally:
        dist.destroy_process_group()


def test_what_stays_refused():
    from fbinet_common import CASES, weights
    from yond_public_amd import _lib as L
    from yond_public_amd import archs as A
    from yond_public_amd.train import TrainStep
    args, _ = CASES['a']
    fbi = A.FBI_Net(dict(args))
    fbi.load_state_dict({k: torch.as_tensor(v) for k, v in weights(args, 3).items()})
    ts = TrainStep(fbi.to(DEV).train(), graph=False)
    x = torch.rand((1, 1, 16, 16), device=DEV)
    with pytest.raises(NotImplementedError, match="FBI_Net"):
        ts.step(x, x)
    net = make('bn', 2)
    with pytest.raises(L.YondHipError, match="train"):
        net(T.batch(1, 0)[0].to(DEV))
