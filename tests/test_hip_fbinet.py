"""GPU: the FBI_Net plug-in (archs.FBI_Net -> fbinet.FBINetPlan) against the reference's own outputs (tests/golden/fbinet.npz, written by
tools/gen_golden_fbinet.py from the reference's archs/comp.py FBI_Net, float32 and float64), its blind spot, the pipeline's `fbi` branch
against the reference's VST_Denoiser, on a stack, through IterDenoise, and in the full-frame driver."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fbinet_common as D
from hip_common import report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPE = {'data_type': 'ANY', 'full_est': True, 'est_type': 'simple+full', 'k': 29, 'full_dn': True, 'vst_type': 'exact', 'bias_corr': 'pre',
        'denoiser_type': 'fbi', 'iter': 'iter', 'max_iter': 1, 'clip': False}          # the runfile's pipeline section


def case(g, name):
    args, shape = D.CASES[name]
    sd = D.weights(args, D.case_seed(g["w_seed"], name))
    x = D.case_input(shape, D.case_seed(g["x_seed"], name))
    return D.build(args, sd, DEV), x


def forward(net, x):
    with torch.no_grad():
        y = net(x.to(DEV))
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_fbinet_matches_reference_float32(golden, name):
    """The bound tests/test_hip_net.py applies to the U-Nets: max |delta| <= 1e-4 max(1, max |ref|)."""
    g = golden("fbinet")
    net, x = case(g, name)
    plan = net._get_plan(torch.device(DEV))
    assert not plan.uses_half_operands()
    plan.prof = []
    y = forward(net, x)
    tags, plan.prof = [p[0] for p in plan.prof], None
    L_ = D.CASES[name][0]['num_of_layers']
    assert tags == (["fbi_first_kernel", "fbi_rm_kernel", "fbi_tapconv_kernel<0>", "fbi_rm_kernel"] + ["fbi_tapconv_kernel<1>", "fbi_rm_kernel"] * (L_ - 2)
                    + ["fbi_rm_kernel", "fbi_out_kernel"]), tags
    ref = g[f"y32_{name}"]
    assert y.shape == ref.shape and y.dtype == np.float32
    assert report(f"FBI_Net ({name}) vs reference float32", y, ref) <= 1e-4 * max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_fbinet_error_against_float64_beside_the_reference(golden, name):
    """Against the reference's float64 output: the HIP forward's largest error is no more than twice the float32 reference's own plus one
    float32 ulp of max |ref| (exact fp32 products, fp32 accumulation in another order)."""
    g = golden("fbinet")
    net, x = case(g, name)
    y = forward(net, x)
    y64 = D.ref64(g, name)
    e_hip = float(np.abs(y.astype(np.float64) - y64).max())
    e_ref = float(np.abs(g[f"y32_{name}"].astype(np.float64) - y64).max())
    ulp = float(np.spacing(np.float32(np.abs(y64).max())))
    print(f"[fbinet] ({name}) max |HIP - f64| = {e_hip:.3e}, max |reference f32 - f64| = {e_ref:.3e}, ratio {e_hip / e_ref:.2f}, ulp(max |ref|) = {ulp:.3e}")
    assert e_hip <= 2.0 * e_ref + ulp


def test_fbinet_flops_and_plan_key():
    args = D.fbi_args()
    net = D.build(args, D.weights(args, 1), DEV)
    plan = net._get_plan(torch.device(DEV))
    per_pixel = plan.flops(1, 1, 1) / 4 / 2
    assert per_pixel == 8 * 64 + (9 + 15 * 5) * 64 * 64 + 18 * 2 * 64 * 64 + 2 * 64          # 0.49 M MAC per pixel
    assert net._get_plan(torch.device(DEV)) is plan
    with torch.no_grad():
        net.activation.weight.mul_(0.5)                                                      # an in-place write: the plan is rebuilt
    assert net._get_plan(torch.device(DEV)) is not plan


def test_fbinet_blind_spot_on_the_gpu():
    """res False: the output at a pixel does not depend on the input there -- bit for bit (no masked product is computed), for a pixel
    in a corner, on a tile seam and in the interior; other pixels change."""
    from yond_public_amd import _lib as L
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    L.check(L.load().yond_fbi_tile(ctypes.byref(th), ctypes.byref(tw)), "yond_fbi_tile")
    args = D.fbi_args(nf=32, num_of_layers=5, res=False, output_channel=1)
    net = D.build(args, D.weights(args, 11), DEV)
    H, W = 2 * th.value + 6, 2 * tw.value + 6
    x = D.case_input((1, 1, H, W), 12)
    y0 = forward(net, x)
    for py, px in [(0, 0), (H - 1, W - 1), (th.value - 1, tw.value), (th.value, tw.value - 1), (th.value + 3, tw.value + 5)]:
        x1 = x.clone()
        x1[0, 0, py, px] += 0.5
        y1 = forward(net, x1)
        assert y1[0, 0, py, px].tobytes() == y0[0, 0, py, px].tobytes(), (py, px)
        assert int((y1 != y0).sum()) >= 1


def vst_net(g):
    args = dict(D.CASES['a'][0])
    return D.build(args, D.vst_weights(args, int(g["vst_seed"])), DEV), args


def test_fbinet_behind_the_vst_matches_reference(golden):
    """pipeline.VST_Denoiser(denoiser='fbi') against the reference's own VST_Denoiser, to the tolerance of the existing vst_denoiser cases."""
    from yond_public_amd import pipeline as P
    g = golden("fbinet")
    net, args = vst_net(g)
    dn = P.VST_Denoiser(torch.from_numpy(D.vst_frame()).to(DEV), D.vst_params(), net, args, bias_corr='pre', denoiser='fbi').cpu().numpy()
    assert dn.shape == g["dn_vst"].shape
    assert report("FBI_Net VST_Denoiser vs reference", dn, g["dn_vst"]) <= 1e-4


def test_fbinet_stack_equals_single_calls(golden):
    """A stack of two different frames (each with its own minimum and maximum) equals the two single calls."""
    from yond_public_amd import pipeline as P
    net, args = vst_net(golden("fbinet"))
    frames = torch.stack([torch.from_numpy(D.synth_noisy(96, 128, 4.0, 6.0, 61 + i)[0] * np.float32(1.0 - 0.3 * i)) for i in range(2)]).to(DEV)
    p = D.vst_params()
    lut = P.get_bias(np.float32(frames.max().item()) * np.float32(959.0), p['sigma'], p['gain'], device=torch.device(DEV))
    both = P.VST_Denoiser(frames, p, net, args, bias_corr='pre', bias_func=lut, denoiser='fbi')
    for i in range(2):
        one = P.VST_Denoiser(frames[i], p, net, args, bias_corr='pre', bias_func=lut, denoiser='fbi')
        assert torch.equal(both[i], one)
    assert not torch.equal(both[0], both[1])


def test_fbinet_keeps_the_device_chains_off():
    from yond_public_amd import pipeline as P
    net, args = vst_net(np.load(os.path.join(ROOT, "tests", "golden", "fbinet.npz")))
    lr = torch.zeros((96, 128), device=DEV)
    blocks = torch.zeros((32, 256, 256), device=DEV)
    other = dict(PIPE, denoiser_type='unetn')
    assert P.chain_applies(lr, net, args, other) and not P.chain_applies(lr, net, args, PIPE)
    assert P.stream_applies(other) and not P.stream_applies(PIPE)
    sidd, sidd_fbi = dict(other, full_dn=False), dict(PIPE, full_dn=False)
    assert P.chain_applies_sidd(blocks, None, net, args, sidd, {}) and not P.chain_applies_sidd(blocks, None, net, args, sidd_fbi, {})


def test_fbinet_iterdenoise_round_1_is_vst_denoiser_at_its_estimate(golden):
    from yond_public_amd import pipeline as P
    net, args = vst_net(golden("fbinet"))
    frame = torch.from_numpy(D.vst_frame()).to(DEV)
    res = P.IterDenoise(frame, net, args, PIPE)
    assert len(res['raw_dns']) >= 1 and all(bool(torch.isfinite(r).all()) for r in res['raw_dns'])
    p = dict(P.default_params())
    p['gain'], p['sigma'] = res['params'][0]
    want = P.VST_Denoiser(frame, p, net, args, bias_corr='pre', vst_type='exact', clip01=True, denoiser='fbi')
    assert torch.equal(res['raw_dns'][0], want)
    got = list(P.denoise_stream(iter([frame]), net, args, PIPE))
    assert len(got) == 1 and torch.equal(got[0]['raw_dns'][0], res['raw_dns'][0])


def test_fbinet_and_fbi_need_each_other(golden):
    from hip_common import ARCHS, make_net
    from yond_public_amd import pipeline as P
    from yond_public_amd._lib import YondHipError
    net, args = vst_net(golden("fbinet"))
    frame = torch.from_numpy(D.vst_frame()).to(DEV)
    with pytest.raises(YondHipError, match="'fbi'"):
        P.VST_Denoiser(frame, D.vst_params(), net, args, bias_corr='pre')
    unet, _ = make_net(ARCHS["gru8"], 3)
    with pytest.raises(YondHipError, match="FBI_Net"):
        P.VST_Denoiser(frame, D.vst_params(), unet, ARCHS["gru8"], bias_corr='pre', denoiser='fbi')
    with pytest.raises(NotImplementedError, match="bm3d"):
        P.VST_Denoiser(frame, D.vst_params(), unet, ARCHS["gru8"], bias_corr='pre', denoiser='bm3d')


def test_fbinet_full_frame_driver_runs_the_runfile(tmp_path, monkeypatch):
    """`YOND_any.py -f runfiles/YOND/ANY_simple+full_pre_fbi.yml -m eval --synthetic 2` on small frames: no checkpoint -> procedurally
    filled (weakly denoising) weights; the run completes and reports PSNR / SSIM per frame."""
    import yaml
    from yond_public_amd import YOND_full as Y
    monkeypatch.chdir(tmp_path)
    cfg = yaml.load(open(os.path.join(ROOT, "runfiles", "YOND", "ANY_simple+full_pre_fbi.yml")).read(), Loader=yaml.FullLoader)
    assert cfg['pipeline'] == PIPE
    for sec in ('dst', 'dst_eval', 'dst_test'):
        cfg[sec].update(root_dir=str(tmp_path / "nowhere"), H=192, W=256, ratio_list=[1])
    rf = tmp_path / "fbi.yml"
    rf.write_text(yaml.dump(cfg))
    drv = Y.YOND_Full(['-f', str(rf), '-m', 'eval', '--synthetic', '2'])
    assert type(drv.net).__name__ == 'FBI_Net' and type(drv.dst_eval).__name__ == 'SyntheticFrames'
    res = drv.eval(-1)
    assert res['x1']['count'] == 2 and len(drv.metrics) == 2
    for m in drv.metrics.values():
        assert len(m['psnr']) >= 1 and len(m['ssim']) == len(m['psnr'])
        assert np.isfinite(m['psnr']).all() and np.isfinite(m['ssim']).all() and m['psnr'][-1] > 20.0
    log = open(tmp_path / "logs" / f"log_{cfg['method_name']}.log").read()
    assert "PSNR=" in log and "SSIM=" in log
