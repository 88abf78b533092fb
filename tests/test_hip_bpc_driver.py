"""GPU: the full-frame driver with the defective-pixel repair -- `YOND_any --bad-pixels auto | FILE.npy` with `--synth-noise 1,2
--synth-defects 40` on a synthetic 256 x 384 frame at ratio 2 (the runfile override of the other driver tests), and the refusals.

The frame the driver makes is rebuilt here with the library called by hand (as tests/test_hip_noisekld_driver.py does): the clean
frame, add_pg_noise keyed by crc32(name), inject_defects keyed by crc32(name + '/defects').  The 40 defects sit at the white level,
ratio * 1.0 = 2, far above the certain-detection bound M + t sqrt(beta1 M + beta2) of the driver's own estimate (asserted below), so
every one must be found; the false detections must be exactly those of the NumPy model on the same frame and estimate.

The noise level of the PSNR sign check.  What the repair does to the input does not depend on it: the repaired run's PSNR is the
clean-input run's at every level measured (below, asserted to 0.01 dB: 40 of 98,304 pixels hold a median instead of their own noisy
value, a change of the MSE of under 1e-3 of it).  What the DEFECTS do to the unrepaired run does: besides their own error they disturb
the pipeline's estimates, and with the synthetic denoising weights of a checkout without a checkpoint a wrong estimate can raise the
PSNR.  At K, sigma = 4, 6 the second round's collaborative estimate of the unrepaired frame is off by 50 % / 170 % (12 % / 15 % on
the clean one) and the unrepaired run scores 34.18 dB against 33.56 dB clean and 33.56 dB repaired: the sign is the estimator's, not
the defects'.  At 2,3, 1,2 and 0.5,1 the second round's estimate is the clean frame's within 1 % and the defects' own error shows:
last-round PSNR clean / defects left in / repaired = 34.204 / 34.110 / 34.203, 34.465 / 34.242 / 34.462, 34.251 / 34.079 / 34.251.
The test runs at 1,2, inside the range where the comparison measures the defects.  With 90 such defects on this small frame (a
density of 1e-3, far above a real sensor's) the run stops in the bias LUT (YOND_EINVAL) with and without `--bad-pixels auto`: the
blind estimates of so defective a frame are no noise model.  That was seen once at each level and not looked into.

Without the flags the driver takes the parent's path: the frame is handed to the pipeline as it was made, bit for bit, the new keys
are absent, and the outputs are those of pipeline.IterDenoise on that frame -- compared as two runs of the same pipeline compare
(tests/test_hip_noisekld_driver.py: equal up to the order of the estimator's atomic float sums, rtol 1e-6 on every round's PSNR and
SSIM; for the frames, whose values lie in [0, 1], an absolute 1e-5).
"""
import os
import zlib

import numpy as np
import pytest
import yaml

import bpc_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 256, 384
RATIO = 2
N_DEFECTS = 40
NOISE = '1,2'
K_DN, SIGMA_DN = 1.0, 2.0


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


def test_driver_bad_pixels(tmp_path, monkeypatch, capsys):
    import torch
    from yond_public_amd import YOND_full as Y
    from yond_public_amd import YOND_SIDD as YS
    from yond_public_amd import bpc as BP
    from yond_public_amd import pgnoise as PG
    from yond_public_amd import pipeline as P
    monkeypatch.chdir(tmp_path)
    rf = _runfile(tmp_path, "any.yml")
    base = ['-f', rf, '-m', 'eval', '--synthetic', '1', '--synth-noise', NOISE]
    plain_keys = {'psnr', 'ssim', 'reg', 'true', 'rel_err'}

    # the frame the driver makes, by hand
    frames = Y.SyntheticFrames(1, H, W, clean_only=True)
    frames.change_eval_ratio(ratio=RATIO)
    item = frames[0]
    name = item['name']
    clean = torch.from_numpy(item['hr']).cuda()

    # the flags off: the parent's path
    plain, in0, out0, log0 = _run(Y, base, capsys)
    assert plain.bad_pixels is None and plain.synth_defects is None and 'bad_pixels' not in plain.pipe
    wp, bl = float(plain.dst.get('wp', 1023)), float(plain.dst.get('bl', 64))
    noisy = PG.add_pg_noise(clean, K_DN, SIGMA_DN, wp - bl, zlib.crc32(name.encode()), [0], exposure=1.0 / RATIO)
    assert set(plain.metrics) == {name} and set(plain.metrics[name]) == plain_keys
    assert "bad pixels" not in log0 and "injected" not in log0
    assert torch.equal(in0[name], noisy)                                 # handed over as it was made
    p = dict(plain.pipe)
    p.update({'wp': wp, 'bl': bl, 'ratio': RATIO, 'gain': 1, 'sigma': 0, 'scale': (wp - bl) / RATIO})
    by_hand = P.IterDenoise(noisy, plain.net, plain.arch, plain.pipe, p=p, device=plain.device, biaslut=plain.biaslut,
                            est={'est_net': plain.est_net.get('est_net'), 'est_args': plain.est_args})
    err = float((by_hand['raw_dns'][-1] - out0[name]).abs().max())
    print(f"[bpc driver] flags off: max |driver - IterDenoise by hand| = {err:.3e}")
    assert err <= 1e-5
    hr = clean.clamp(0, 1)
    assert len(plain.metrics[name]['psnr']) == len(by_hand['raw_dns']) == 2
    for it, dn in enumerate(by_hand['raw_dns']):                         # the metrics, round by round, at that test's rtol
        ps, ss = P.block_metrics(dn, hr, bh=H, bw=W)
        ps, ss = float(np.mean(ps)), float(np.mean(ss))
        with capsys.disabled():
            print(f"\n[bpc driver] flags off, round {it}: PSNR {plain.metrics[name]['psnr'][it]!r} / by hand {ps!r}, SSIM {plain.metrics[name]['ssim'][it]!r} / {ss!r}")
        assert np.isclose(plain.metrics[name]['psnr'][it], ps, rtol=1e-6, atol=0)
        assert np.isclose(plain.metrics[name]['ssim'][it], ss, rtol=1e-6, atol=0)

    # defects left in: the metrics say so, and the PSNR is what the repair has to beat
    broken, in1, _, log1 = _run(Y, base + ['--synth-defects', str(N_DEFECTS)], capsys)
    defective, truth = BP.inject_defects(noisy, N_DEFECTS, zlib.crc32((name + '/defects').encode()), None, ratio=RATIO)
    assert truth.shape == (N_DEFECTS, 2) and bool((defective[truth[:, 0], truth[:, 1]] == float(RATIO)).all())
    assert torch.equal(in1[name], defective) and torch.equal(torch.from_numpy(item['hr']), torch.from_numpy(frames[0]['hr']))
    assert broken.metrics[name]['defects'] == {'n': N_DEFECTS} and 'bad_pixels' not in broken.metrics[name]
    assert f"{N_DEFECTS} injected defects left in" in log1

    # --bad-pixels auto
    auto, in2, _, log2 = _run(Y, base + ['--synth-defects', str(N_DEFECTS), '--bad-pixels', 'auto'], capsys)
    assert auto.bad_pixels == ('auto', 6.0)
    m = auto.metrics[name]
    assert set(m) == plain_keys | {'bad_pixels', 'bad_pixels_model', 'defects'} and set(m['bad_pixels']) == {'hot', 'cold'}
    beta1, beta2, t = m['bad_pixels_model']
    assert t == 6.0 and beta1 > 0 and beta2 >= 0
    host = defective.cpu().numpy()
    undisturbed_max = float(noisy.max())
    bound = M.certain_bound(undisturbed_max, beta1, beta2, t)
    print(f"[bpc driver] estimate beta1 {beta1:.4e}, beta2 {beta2:.4e}; certain above {bound:.4f}, defects at {RATIO}; {m['bad_pixels']}, {m['defects']}")
    assert float(RATIO) > bound
    want, winfo = M.detect_and_repair(host, beta1, beta2, t)
    truth_set = {(int(r), int(c)) for r, c in truth}
    model_set = {(int(r), int(c)) for r, c in winfo['points']}
    assert m['defects'] == {'n': N_DEFECTS, 'found': N_DEFECTS, 'false': len(model_set - truth_set)}
    assert m['bad_pixels'] == {'hot': winfo['hot'], 'cold': winfo['cold']}
    assert np.array_equal(in2[name].cpu().numpy(), want)                 # the pipeline is handed the model's repaired frame
    assert f"found {N_DEFECTS} / {N_DEFECTS} injected" in log2 and "bad pixels hot=" in log2
    psnr_broken, psnr_auto = broken.metrics[name]['psnr'][-1], m['psnr'][-1]
    print(f"[bpc driver] PSNR of the last round: clean input {plain.metrics[name]['psnr'][-1]:.3f}, defects left in {psnr_broken:.3f}, repaired {psnr_auto:.3f}")
    assert psnr_auto > psnr_broken
    assert abs(psnr_auto - plain.metrics[name]['psnr'][-1]) < 0.01       # the repair gives the pipeline back its clean-sensor input

    # --bad-pixels FILE.npy with the truth list: repair_bad_pixels on the driver's own input frame; auto:T and the runfile key
    np.save(tmp_path / "bad.npy", truth)
    rf2 = _runfile(tmp_path, "any_bp.yml", bad_pixels=str(tmp_path / "bad.npy"))
    listed, in3, _, log3 = _run(Y, ['-f', rf2, '-m', 'eval', '--synthetic', '1', '--synth-noise', NOISE, '--synth-defects', str(N_DEFECTS), '--save', 'f32'], capsys)
    assert listed.bad_pixels == ('list', str(tmp_path / "bad.npy")) and 'bad_pixels' not in listed.pipe
    assert torch.equal(in3[name], BP.repair_bad_pixels(defective, truth))
    assert np.array_equal(in3[name].cpu().numpy(), M.repair_list(host, truth))
    assert listed.metrics[name]['bad_pixels'] == {'hot': N_DEFECTS, 'cold': 0}
    assert listed.metrics[name]['defects'] == {'n': N_DEFECTS, 'found': N_DEFECTS, 'false': 0}
    assert listed.metrics[name]['psnr'][-1] > psnr_broken
    import json
    side = json.load(open(os.path.join(listed.save_dir, name + '.json')))
    assert side['bad_pixels'] == {'hot': N_DEFECTS, 'cold': 0} and 'bad_pixels_points' not in side
    over, in4, _, _ = _run(Y, ['-f', rf2, '-m', 'eval', '--synthetic', '1', '--synth-noise', NOISE, '--synth-defects', f'{N_DEFECTS},1.5',
                               '--bad-pixels', 'auto:5', '--save', 'f32'], capsys)
    assert over.bad_pixels == ('auto', 5.0) and over.synth_defects == (N_DEFECTS, 1.5)                # the flag overrides the runfile
    assert over.metrics[name]['defects']['found'] == N_DEFECTS and over.metrics[name]['bad_pixels_model'][2] == 5.0
    side = json.load(open(os.path.join(over.save_dir, name + '.json')))
    assert side['bad_pixels'] == over.metrics[name]['bad_pixels']
    assert truth_set <= {tuple(q) for q in side['bad_pixels_points']} and len(side['bad_pixels_points']) <= BP.MAX_SAVED_POINTS

    # a list that does not fit the frames is refused, frame by frame
    np.save(tmp_path / "wide.npy", np.array([[0, W]]))
    with pytest.raises(ValueError):
        Y.YOND_Full(base + ['--bad-pixels', str(tmp_path / "wide.npy")]).eval(-1)
    capsys.readouterr()

    # the refusals
    for flags in (['--bad-pixels', 'auto'], ['--synth-defects', '10'], ['--bad-pixels', str(tmp_path / "bad.npy")]):
        with pytest.raises(SystemExit):
            YS.YOND_SIDD(flags)                                          # YOND_SIDD, and YOND_DND, which is YOND_SIDD with another runfile
        with pytest.raises(SystemExit):
            YS.YOND_SIDD(['-f', os.path.join(ROOT, "runfiles", "YOND", "DND_simple+full_pre_grumix.yml")] + flags)
    with pytest.raises(SystemExit):
        Y.YOND_Full(['-f', rf, '-m', 'eval', '--synthetic', '1', '--synth-defects', '10'])             # no noise flag
    with pytest.raises(SystemExit):
        Y.YOND_Full(base + ['--bad-pixels', 'median'])
