"""GPU: the DnCNN plug-in (archs.DnCNN -> dncnn.DnCNNPlan) against the reference's own outputs (tests/golden/dncnn.npz, written by
tools/gen_golden_dncnn.py from the reference's archs/comp.py DnCNN in .eval() mode, float32 and float64), behind the VST, on the
fp32-input MFMA path, through the range guard, on the stream driver and in the full-frame driver."""
import os
import warnings

import numpy as np
import pytest
import torch

import dncnn_common as D
from hip_common import report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def case(g, name, precision=None):
    args, shape = D.CASES[name]
    args = dict(args) if precision is None else dict(args, precision=precision)
    sd = D.weights(args, D.case_seed(g["w_seed"], name))
    x = D.case_input(shape, D.case_seed(g["x_seed"], name))
    return D.build(args, sd, DEV), x


def forward(net, x):
    with warnings.catch_warnings(record=True) as wl:
        warnings.simplefilter("always")
        with torch.no_grad():
            y = net(x.to(DEV))
        torch.cuda.synchronize()
    return y.cpu().numpy(), [w for w in wl if "fp16's range" in str(w.message)]


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_dncnn_matches_reference_float32(golden, name):
    """The bound tests/test_hip_net.py applies to the U-Nets: max |delta| <= 1e-4 max(1, max |ref|)."""
    g = golden("dncnn")
    net, x = case(g, name)
    y, tripped = forward(net, x)
    assert not tripped
    ref = g[f"y32_{name}"]
    assert y.shape == ref.shape and y.dtype == np.float32
    assert report(f"DnCNN ({name}) vs reference float32", y, ref) <= 1e-4 * max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_dncnn_error_against_float64_beside_the_reference(golden, name):
    """Against the reference's float64 output: the HIP forward's largest error is no more than twice the float32 reference's own plus one
    float32 ulp of max |ref|."""
    g = golden("dncnn")
    net, x = case(g, name)
    y, _ = forward(net, x)
    y64 = D.ref64(g, name)
    e_hip = float(np.abs(y.astype(np.float64) - y64).max())
    e_ref = float(np.abs(g[f"y32_{name}"].astype(np.float64) - y64).max())
    ulp = float(np.spacing(np.float32(np.abs(y64).max())))
    print(f"[dncnn] ({name}) max |HIP - f64| = {e_hip:.3e}, max |reference f32 - f64| = {e_ref:.3e}, ratio {e_hip / e_ref:.2f}, ulp(max |ref|) = {ulp:.3e}")
    assert e_hip <= 2.0 * e_ref + ulp


def test_dncnn_behind_the_vst_matches_reference(golden):
    """(e): pipeline.VST_Denoiser with net (a) against the reference's own VST_Denoiser, to the tolerance of the existing vst_denoiser cases."""
    from yond_public_amd import pipeline as P
    g = golden("dncnn")
    args = dict(D.CASES['a'][0])
    net = D.build(args, D.weights(args, int(g["vst_seed"])), DEV)
    dn = P.VST_Denoiser(torch.from_numpy(D.vst_frame()).to(DEV), D.vst_params(), net, args, bias_corr='pre').cpu().numpy()
    assert report("DnCNN VST_Denoiser vs reference", dn, g["dn_vst"]) <= 1e-4


@pytest.mark.parametrize("name", ["a", "b"])
def test_dncnn_fp32_mfma_path(golden, name):
    """precision 'fp32-mfma': every middle layer on the fp32-input MFMA kernels -- the same bounds; and no split-operand launch."""
    g = golden("dncnn")
    net, x = case(g, name, precision='fp32-mfma')
    plan = net._get_plan(torch.device(DEV))
    assert not plan.uses_half_operands()
    plan.prof = []
    y, tripped = forward(net, x)
    tags, plan.prof = [p[0] for p in plan.prof], None
    assert not tripped
    assert tags[0] == "conv_in_kernel" and tags[-1] == "conv3x3_out4_kernel" and len(tags) == D.CASES[name][0]['depth']
    assert all(t.startswith(("conv_wino_kernel", "conv_mfma_kernel")) and "/f16" not in t for t in tags[1:-1]), tags
    ref = g[f"y32_{name}"]
    assert report(f"DnCNN ({name}) fp32-mfma vs reference float32", y, ref) <= 1e-4 * max(1.0, float(np.abs(ref).max()))
    y64 = D.ref64(g, name)
    e_hip, e_ref = float(np.abs(y - y64).max()), float(np.abs(ref.astype(np.float64) - y64).max())
    print(f"[dncnn] ({name}) fp32-mfma: max |HIP - f64| = {e_hip:.3e}, reference {e_ref:.3e}")
    assert e_hip <= 2.0 * e_ref + float(np.spacing(np.float32(np.abs(y64).max())))


def test_dncnn_default_path_runs_the_split_kernels_and_the_new_last_layer(golden):
    g = golden("dncnn")
    net, x = case(g, "a")
    plan = net._get_plan(torch.device(DEV))
    assert plan.uses_half_operands()
    plan.prof = []
    forward(net, x)
    tags, plan.prof = [p[0] for p in plan.prof], None
    assert tags[0] == "conv_in_kernel" and tags[-1] == "conv3x3_out4_kernel"
    assert all(t.startswith("conv_split_kernel<1,") and t.endswith(",2>") for t in tags[1:-1]), tags


def test_dncnn_fp16_path(golden):
    """precision 'fp16' works through the h-only split kernels (algo 4): >= 55 dB from the float32 reference on the O(1) output, as the
    U-Nets' fp16 path is held."""
    g = golden("dncnn")
    net, x = case(g, "a", precision='fp16')
    y, _ = forward(net, x)
    ref = g["y32_a"].astype(np.float64)
    psnr = 10 * np.log10(1.0 / max(float(np.mean((y - ref) ** 2)), 1e-30))
    print(f"[dncnn] (a) fp16 path vs float32 reference: {psnr:.1f} dB")
    assert np.isfinite(y).all() and psnr >= 55.0


def test_dncnn_train_mode_with_batchnorm_is_refused(golden):
    from yond_public_amd._lib import YondHipError
    g = golden("dncnn")
    net, x = case(g, "a")
    net.train()
    with pytest.raises(YondHipError, match="train"):
        net(x.to(DEV))
    net.eval()
    assert np.isfinite(forward(net, x)[0]).all()
    nobn, xb = case(g, "b")
    nobn.train()                                              # without BatchNorm layers the mode changes nothing
    assert np.array_equal(forward(nobn, xb)[0], forward(nobn.eval(), xb)[0])


def test_dncnn_range_guard_returns_the_fp32_mfma_result():
    """depth 4, nf 32 on 1x4x16x16: the first BatchNorm's gamma x 1e6, the next convolution's weights / 1e6 -- the tensor between them
    leaves fp16's range, so the guard must trip, the result must be the fp32-input MFMA path's (bit for bit) and match a float64 torch
    model of the same weights within the float32 networks' bound."""
    args = D.dn_args(depth=4, nf=32, use_bn=True, res=True)
    sd = D.weights(args, 31)
    sd['dncnn.3.weight'] = sd['dncnn.3.weight'] * 1e6
    sd['dncnn.5.weight'] = sd['dncnn.5.weight'] / 1e6
    x = D.case_input((1, 4, 16, 16), 32)
    ref = D.torch_model64(args, sd, x).numpy()
    assert np.isfinite(ref).all() and float(np.abs(ref).max()) < 100.0
    net = D.build(args, sd, DEV)
    y, tripped = forward(net, x)
    assert len(tripped) == 1
    assert np.isfinite(y).all()
    assert report("guarded DnCNN vs float64 model", y, ref) <= 1e-4 * max(1.0, float(np.abs(ref).max()))
    strict, t2 = forward(D.build(dict(args, precision='fp32-mfma'), sd, DEV), x)
    assert not t2 and np.array_equal(y, strict)
    # the pipeline's guard (VST_Denoiser) recomputes as well
    from yond_public_amd import pipeline as P
    frame = torch.from_numpy(D.vst_frame()).to(DEV)
    with warnings.catch_warnings(record=True) as wl:
        warnings.simplefilter("always")
        dn = P.VST_Denoiser(frame, D.vst_params(), net, args, bias_corr='pre')
        raw = P.VST_Denoiser(frame, D.vst_params(), net, args, bias_corr='pre', guard=False)
    assert any("fp16's range" in str(w.message) for w in wl) and bool(torch.isfinite(dn).all())
    mfma = P.VST_Denoiser(frame, D.vst_params(), D.build(dict(args, precision='fp32-mfma'), sd, DEV), args, bias_corr='pre')
    assert torch.equal(dn, mfma)
    assert not bool(torch.isfinite(raw).all()) or float((raw - dn).abs().max()) > 1e-3


def test_dncnn_stream_driver_equals_iterdenoise():
    """denoise_stream on two 128 x 192 frames equals per-frame IterDenoise, as tests/test_hip_pipeline.py asserts for the U-Nets."""
    import yond_public_amd.pipeline as P
    import yond_public_amd.synthetic as S
    args = D.dn_args(depth=5, nf=32)
    net = D.DnCNN(dict(args))
    net.load_state_dict(S.denoising_state_dict(net, 0))
    net = net.to(DEV).eval()
    frames = [torch.from_numpy(S.synth_noisy(128, 192, 3.0 + i, 5.0 + 2 * i, 10 + i)[0]).to(DEV) for i in range(2)]
    for it in ('once', 'iter'):
        pipe = {'k': 29, 'vst_type': 'exact', 'bias_corr': 'pre', 'iter': it, 'max_iter': 1, 'full_dn': True}
        seq = [P.IterDenoise(f, net, args, pipe) for f in frames]
        got = list(P.denoise_stream(iter(frames), net, args, pipe))
        torch.cuda.synchronize()
        assert len(got) == len(seq) == 2
        for a_, b_ in zip(got, seq):
            assert len(a_['raw_dns']) == len(b_['raw_dns'])
            assert np.allclose(np.asarray(a_['regs'], np.float64), np.asarray(b_['regs'], np.float64), rtol=1e-9, atol=0)
            for u, v in zip(a_['raw_dns'], b_['raw_dns']):
                assert bool(torch.isfinite(u).all()) and float((u - v).abs().max()) <= 5e-6


def test_dncnn_full_frame_driver_runs_the_runfile(tmp_path, monkeypatch):
    """`YOND_any.py -f runfiles/YOND/ANY_simple+full_pre_dncnn.yml -m eval --synthetic 2` on small frames: no checkpoint -> procedurally
    filled (weakly denoising) weights; the run completes and reports PSNR / SSIM per frame."""
    import yaml
    from yond_public_amd import YOND_full as Y
    monkeypatch.chdir(tmp_path)
    cfg = yaml.load(open(os.path.join(ROOT, "runfiles", "YOND", "ANY_simple+full_pre_dncnn.yml")).read(), Loader=yaml.FullLoader)
    assert cfg['arch'] == dict(name='DnCNN', in_nc=4, out_nc=4, nf=64, depth=17, use_bn=True, res=True)
    for sec in ('dst', 'dst_eval', 'dst_test'):
        cfg[sec].update(root_dir=str(tmp_path / "nowhere"), H=192, W=256, ratio_list=[1])
    rf = tmp_path / "dncnn.yml"
    rf.write_text(yaml.dump(cfg))
    drv = Y.YOND_Full(['-f', str(rf), '-m', 'eval', '--synthetic', '2'])
    assert type(drv.net).__name__ == 'DnCNN' and type(drv.dst_eval).__name__ == 'SyntheticFrames'
    res = drv.eval(-1)
    assert res['x1']['count'] == 2 and len(drv.metrics) == 2
    for m in drv.metrics.values():
        assert len(m['psnr']) >= 1 and len(m['ssim']) == len(m['psnr'])
        assert np.isfinite(m['psnr']).all() and np.isfinite(m['ssim']).all() and m['psnr'][-1] > 20.0
    log = open(tmp_path / "logs" / f"log_{cfg['method_name']}.log").read()
    assert "PSNR=" in log and "SSIM=" in log
