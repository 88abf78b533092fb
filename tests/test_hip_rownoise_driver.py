"""GPU: the full-frame driver with the row-noise removal -- `YOND_any --camera-noise code=pr,K=1,sigGs=2,sigR=3 --row-denoise
sc=10,ss=9,d=25` on a synthetic 256 x 384 frame at ratio 2 (the runfile override of the other driver tests), and the refusals.
(Shot noise K = 1, Gaussian read noise of 2 DN, row noise of 3 DN.  In the reference's letters the Gaussian read noise is the code
WITHOUT `g` -- `g` is the Tukey-lambda term and needs sigTL and lam, so `--camera-noise` refuses code=pgr with these keys.)

The frame the driver makes is rebuilt here with the library called by hand (as tests/test_hip_bpc_driver.py does): the clean frame,
add_camera_noise keyed by crc32(name).  The frame handed to the pipeline must be tests/rownoise_model.py applied to it, within the
end-to-end bound of tests/test_hip_rownoise.py (half a float32 ulp plus e2e_band), with sigma_color converted to the frame's units,
sc * ratio / (wp - bl).

The condition that shows it works: the standard deviation over rows of the row means of (input - clean) is, after the step, at most 0.5
of what it was before.  The NumPy model alone gives 0.24-0.27 on this generator, size and level, so the cap is met with room to spare;
a step that does nothing gives 1.0, the wrong sign about 1.9.  The reported sigma of the removed offsets lies within [0.6, 1.1] * sigR:
the model gives 2.4-2.6 of 3, the filter keeps about 1 / N_eff of the variance.

No sign of the PSNR is asserted: with the synthetic denoising weights of a checkout without a checkpoint such a sign measures the
estimator (tests/test_hip_bpc_driver.py explains why); both values are logged.

Without the flag the driver takes the parent's path: the frame is handed on bit for bit as it was made, `row_noise` is absent, and the
outputs are those of pipeline.IterDenoise on that frame, compared as two runs of the same pipeline compare (rtol 1e-6 on every round's
PSNR and SSIM, an absolute 1e-5 on the frames).
"""
import json
import os
import zlib

import numpy as np
import pytest
import yaml

import rownoise_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 256, 384
RATIO = 2
SIG_R = 3.0
CAM = f'code=pr,K=1,sigGs=2,sigR={SIG_R:g}'
SPEC = 'sc=10,ss=9,d=25'
SC_DN, SS, D = 10.0, 9.0, 25


def _runfile(tmp_path, name, **pipeline):
    cfg = yaml.load(open(os.path.join(ROOT, "runfiles", "YOND", "ANY_simple+full_pre_grumix.yml")).read(), Loader=yaml.FullLoader)
    for sec in ('dst', 'dst_eval', 'dst_test'):
        cfg[sec].update(root_dir=str(tmp_path / "nowhere"), H=H, W=W, ratio_list=[RATIO])
    cfg['pipeline'].update(pipeline)
    rf = tmp_path / name
    rf.write_text(yaml.dump(cfg))
    return str(rf)


def _run(Y, args, capsys):
    """(driver, {name: input frame as handed to the pipeline}, {name: last round's output}, log)."""
    drv = Y.YOND_Full(args)
    inputs, outputs = {}, {}
    drv.on_input = lambda name, lr: inputs.__setitem__(name, lr.clone())
    drv.on_result = lambda name, res: outputs.__setitem__(name, res['raw_dns'][-1].clone())
    drv.eval(-1)
    return drv, inputs, outputs, capsys.readouterr().out


def _banding(frame, clean):
    """The standard deviation over rows of the row means of (frame - clean)."""
    return float((frame.double() - clean.double()).mean(dim=1).std())


def test_driver_row_denoise(tmp_path, monkeypatch, capsys):
    import torch
    from yond_public_amd import YOND_full as Y
    from yond_public_amd import YOND_SIDD as YS
    from yond_public_amd import camnoise as CN
    from yond_public_amd import pipeline as P
    from yond_public_amd import rownoise as RN
    monkeypatch.chdir(tmp_path)

    def say(text):                                                       # (past the capture that _run reads the driver's log from)
        with capsys.disabled():
            print("\n" + text, end="")
    rf = _runfile(tmp_path, "any.yml")
    base = ['-f', rf, '-m', 'eval', '--synthetic', '1', '--camera-noise', CAM]
    plain_keys = {'psnr', 'ssim', 'reg', 'true', 'rel_err'}

    # the frame the driver makes, by hand
    frames = Y.SyntheticFrames(1, H, W, clean_only=True)
    frames.change_eval_ratio(ratio=RATIO)
    item = frames[0]
    name = item['name']
    clean = torch.from_numpy(item['hr']).cuda()

    # the flag off: the parent's path
    plain, in0, out0, log0 = _run(Y, base, capsys)
    assert plain.row_denoise is None and 'row_denoise' not in plain.pipe
    wp, bl = float(plain.dst.get('wp', 1023)), float(plain.dst.get('bl', 64))
    spec = CN.camera_noise_arg(CAM)
    noisy = CN.add_camera_noise(clean, dict(spec, wp=wp, bl=bl), spec['code'], wp - bl, zlib.crc32(name.encode()), [0], layout=CN.LAYOUT_BAYER,
                                ratio=float(RATIO), mfm=spec['mfm'], clip=spec['clip'])
    assert set(plain.metrics) == {name} and set(plain.metrics[name]) == plain_keys and 'row_noise' not in plain.metrics[name]
    assert "row noise" not in log0
    assert torch.equal(in0[name], noisy)                                 # handed over as it was made, bit for bit
    p = dict(plain.pipe)
    p.update({'wp': wp, 'bl': bl, 'ratio': RATIO, 'gain': 1, 'sigma': 0, 'scale': (wp - bl) / RATIO})
    by_hand = P.IterDenoise(noisy, plain.net, plain.arch, plain.pipe, p=p, device=plain.device, biaslut=plain.biaslut,
                            est={'est_net': plain.est_net.get('est_net'), 'est_args': plain.est_args})
    err = float((by_hand['raw_dns'][-1] - out0[name]).abs().max())
    say(f"[rownoise driver] flag off: max |driver - IterDenoise by hand| = {err:.3e}")
    assert err <= 1e-5
    hr = clean.clamp(0, 1)
    assert len(plain.metrics[name]['psnr']) == len(by_hand['raw_dns']) == 2
    for it, dn in enumerate(by_hand['raw_dns']):
        ps, ss = P.block_metrics(dn, hr, bh=H, bw=W)
        ps, ss = float(np.mean(ps)), float(np.mean(ss))
        say(f"[rownoise driver] flag off, round {it}: PSNR {plain.metrics[name]['psnr'][it]!r} / by hand {ps!r}, SSIM {plain.metrics[name]['ssim'][it]!r} / {ss!r}")
        assert np.isclose(plain.metrics[name]['psnr'][it], ps, rtol=1e-6, atol=0)
        assert np.isclose(plain.metrics[name]['ssim'][it], ss, rtol=1e-6, atol=0)

    # --row-denoise: the pipeline is handed the model's frame
    host = noisy.cpu().numpy()
    sc_units = SC_DN * RATIO / (wp - bl)
    dn_per_unit = (wp - bl) / RATIO

    def check(inp, per, what):
        _, off, z = M.row_denoise(host, per, D, sc_units, SS)
        got = inp.cpu().numpy()
        lim = 0.5 * np.spacing(np.abs(got)).astype(np.float64) + M.per_pixel(M.e2e_band(host, per, D, sc_units, SS), W)
        err = np.abs(got.astype(np.float64) - z)
        say(f"[rownoise driver] {what}: max |input - model| = {float(err.max()):.3e}, max err / bound = {float((err / lim).max()):.3f}")
        assert (err <= lim).all()
        return off

    on, in1, _, log1 = _run(Y, base + ['--row-denoise', SPEC, '--save', 'f32'], capsys)
    assert on.row_denoise == {'sc': SC_DN, 'ss': SS, 'd': D, 'per': 'row'} and 'row_denoise' not in on.pipe
    off = check(in1[name], M.ROW, "row")
    before, after = _banding(noisy, clean), _banding(in1[name], clean)
    say(f"[rownoise driver] banding (std over rows of the row means of input - clean), frame units: before {before:.5e}, after {after:.5e}, "
          f"ratio {after / before:.3f}; in DN at capture {before * dn_per_unit:.3f} -> {after * dn_per_unit:.3f}")
    assert after <= 0.5 * before
    m = on.metrics[name]
    assert set(m) == plain_keys | {'row_noise'} and set(m['row_noise']) == {'sigma', 'max'}
    say(f"[rownoise driver] reported {m['row_noise']}, injected sigR {SIG_R}")
    assert 0.6 * SIG_R <= m['row_noise']['sigma'] <= 1.1 * SIG_R and m['row_noise']['max'] >= m['row_noise']['sigma']
    assert np.isclose(m['row_noise']['sigma'], float(np.sqrt((off ** 2).mean())) * dn_per_unit, rtol=1e-9)
    assert np.isclose(m['row_noise']['max'], float(np.abs(off).max()) * dn_per_unit, rtol=1e-9)
    assert "row noise removed sigma=" in log1 and f"injected sigR={SIG_R:g}" in log1
    side = json.load(open(os.path.join(on.save_dir, name + '.json')))
    assert side['row_noise'] == m['row_noise']
    assert torch.equal(torch.from_numpy(item['hr']), torch.from_numpy(frames[0]['hr']))      # the ground truth is untouched
    say(f"[rownoise driver] PSNR of the last round: banding left in {plain.metrics[name]['psnr'][-1]:.3f}, removed {m['psnr'][-1]:.3f}")

    # per=plane runs and reports
    plane, in2, _, log2 = _run(Y, base + ['--row-denoise', SPEC + ',per=plane'], capsys)
    assert plane.row_denoise['per'] == 'plane'
    check(in2[name], M.PLANE, "plane")
    mp = plane.metrics[name]['row_noise']
    say(f"[rownoise driver] per=plane: reported {mp}, banding ratio {_banding(in2[name], clean) / before:.3f}")
    assert mp['sigma'] > 0 and np.isfinite(mp['max']) and "row noise removed" in log2

    # the runfile key gives the same frame as the flag; the flag overrides it
    rf2 = _runfile(tmp_path, "any_rn.yml", row_denoise=SPEC)
    keyed, in3, _, _ = _run(Y, ['-f', rf2, '-m', 'eval', '--synthetic', '1', '--camera-noise', CAM], capsys)
    assert keyed.row_denoise == on.row_denoise and 'row_denoise' not in keyed.pipe
    assert torch.equal(in3[name], in1[name]) and keyed.metrics[name]['row_noise'] == m['row_noise']
    over = Y.YOND_Full(['-f', rf2, '-m', 'eval', '--synthetic', '1', '--camera-noise', CAM, '--row-denoise', 'per=plane'])
    assert over.row_denoise == {'sc': 10.0, 'ss': 'auto', 'd': 25, 'per': 'plane'}
    capsys.readouterr()

    # the refusals
    for flags in (['--row-denoise'], ['--row-denoise', SPEC]):
        with pytest.raises(SystemExit):
            YS.YOND_SIDD(flags)                                          # YOND_SIDD, and YOND_DND, which is YOND_SIDD with another runfile
        with pytest.raises(SystemExit):
            YS.YOND_SIDD(['-f', os.path.join(ROOT, "runfiles", "YOND", "DND_simple+full_pre_grumix.yml")] + flags)
    with pytest.raises(SystemExit):
        Y.YOND_Full(base + ['--row-denoise', 'd=24'])


def test_ss_auto_without_an_iso_says_so_once(tmp_path, monkeypatch, capsys):
    """The synthetic items carry no ISO: ss=auto uses ISO 1600 (sigma_space 9) and the log says so, once."""
    import torch
    from yond_public_amd import YOND_full as Y
    monkeypatch.chdir(tmp_path)
    rf = _runfile(tmp_path, "any.yml")
    auto, in_auto, _, log_auto = _run(Y, ['-f', rf, '-m', 'eval', '--synthetic', '2', '--camera-noise', CAM, '--row-denoise'], capsys)
    given, in_given, _, log_given = _run(Y, ['-f', rf, '-m', 'eval', '--synthetic', '2', '--camera-noise', CAM, '--row-denoise', 'ss=9'], capsys)
    assert log_auto.count("carries no ISO") == 1 and "ISO 1600" in log_auto and "carries no ISO" not in log_given
    assert set(in_auto) == set(in_given) and len(in_auto) == 2
    for name in in_auto:
        assert torch.equal(in_auto[name], in_given[name])
