"""GPU: the full-frame driver with the illuminance correction -- `YOND_any --illum-corr frame | cfa` on synthetic frames whose noise
carries a dark bias (`--camera-noise code=pgd,...`), the runfile key pipeline.illum_corr, and the refusals."""
import json
import os

import numpy as np
import pytest
import yaml

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 256, 384
NOISE = 'code=pgd,K=0.5,sigTL=1.0,lam=-0.02,bias=4'                 # a dark bias of 4 DN on every channel
NOISE_CFA = 'code=pgd,K=0.5,sigTL=1.0,lam=-0.02,bias=6/1/2/4'       # ... and one that differs per channel


def _runfile(tmp_path, name, **pipeline):
    cfg = yaml.load(open(os.path.join(ROOT, "runfiles", "YOND", "ANY_simple+full_pre_grumix.yml")).read(), Loader=yaml.FullLoader)
    for sec in ('dst', 'dst_eval', 'dst_test'):
        cfg[sec].update(root_dir=str(tmp_path / "nowhere"), H=H, W=W)
    cfg['pipeline'].update(pipeline)
    rf = tmp_path / name
    rf.write_text(yaml.dump(cfg))
    return str(rf)


def test_driver_illum_corr(tmp_path, monkeypatch, capsys):
    from yond_public_amd import YOND_full as Y
    from yond_public_amd import YOND_SIDD as YS
    from yond_public_amd._lib import YondHipError
    monkeypatch.chdir(tmp_path)
    rf = _runfile(tmp_path, "any.yml")
    base = ['-f', rf, '-m', 'eval', '--synthetic', '1']

    # the synthetic clean frames peak at 0.6: no target is saturated, the gain is taken over the whole frame
    for ratio in (1, 2):
        frames = Y.SyntheticFrames(1, H, W, clean_only=True)
        frames.change_eval_ratio(ratio=ratio)
        hr = frames[0]['hr']
        assert not (np.clip(hr, 0, 1) == 1).any() and hr.max() <= 0.61

    # without the flag: the keys of today, no new log text
    plain = Y.YOND_Full(base + ['--camera-noise', NOISE])
    assert plain.illum_corr == 'off' and 'illum_corr' not in plain.pipe
    res0 = plain.eval(-1)
    out0 = capsys.readouterr().out
    assert "(ic)" not in out0 and "illum" not in out0 and "gain=" not in out0
    n_it = 2
    want = {'count', 'psnr_last', 'ssim_last'} | {f'{k}_iter{it}' for it in range(n_it) for k in ('psnr', 'ssim', 'rel_err_K', 'rel_err_sigma')}
    assert res0 and all(set(red) == want for red in res0.values())
    assert plain.metrics and all(set(m) == {'psnr', 'ssim', 'reg', 'true', 'rel_err', 'bias'} for m in plain.metrics.values())

    # --illum-corr frame
    drv = Y.YOND_Full(base + ['--camera-noise', NOISE, '--illum-corr', 'frame'])
    assert drv.illum_corr == 'frame' and 'illum_corr' not in drv.pipe
    res = drv.eval(-1)
    out = capsys.readouterr().out
    assert "PSNR(ic)=" in out and "SSIM(ic)=" in out and "gain=" in out
    assert any("Iter0:" in line and "PSNR(ic)=" in line and "gain=" in line for line in out.splitlines())
    assert any("Iter_last:" in line and "PSNR(ic)=" in line for line in out.splitlines())
    assert set(drv.metrics) == set(plain.metrics)
    for name, m in drv.metrics.items():
        assert set(m) == {'psnr', 'ssim', 'reg', 'true', 'rel_err', 'bias', 'psnr_ic', 'ssim_ic', 'illum_gain'}
        # the plain metrics stay where they are (two runs of the pipeline: equal up to the order of the estimator's atomic sums)
        assert np.allclose(m['psnr'], plain.metrics[name]['psnr'], rtol=1e-6, atol=0) and np.allclose(m['ssim'], plain.metrics[name]['ssim'], rtol=1e-6, atol=0)
        assert len(m['psnr_ic']) == len(m['ssim_ic']) == len(m['illum_gain']) == len(m['psnr']) >= 1
        assert np.isfinite(m['illum_gain']).all() and np.isfinite(m['psnr_ic']).all() and np.isfinite(m['ssim_ic']).all()
        for it in range(len(m['psnr'])):
            print(f"[illum driver] {name} round {it}: PSNR {m['psnr'][it]:.4f} -> {m['psnr_ic'][it]:.4f}, gain {m['illum_gain'][it]:.6f}")
            assert m['psnr_ic'][it] >= m['psnr'][it] - 1e-4
        assert m['psnr_ic'][-1] > m['psnr'][-1]                                                          # the bias is there to be removed
    for label, red in res.items():
        assert set(red) == want | {'psnr_ic_last', 'ssim_ic_last'} | {f'{k}_ic_iter{it}' for it in range(n_it) for k in ('psnr', 'ssim')}
        assert all(np.isclose(red[k], res0[label][k], rtol=1e-6, atol=0) for k in want)
        names = [n for n in drv.metrics if n.endswith(f"_x{int(label[1:]):02d}")]
        assert names and np.isclose(red['psnr_ic_last'], np.mean([drv.metrics[n]['psnr_ic'][-1] for n in names]), rtol=0, atol=1e-9)

    # --illum-corr cfa with a bias that differs per channel: each channel's own gain fits no worse than the frame's
    frame = Y.YOND_Full(base + ['--camera-noise', NOISE_CFA, '--illum-corr', 'frame'])
    frame.eval(-1)
    cfa = Y.YOND_Full(base + ['--camera-noise', NOISE_CFA, '--illum-corr', 'cfa', '--save', 'f32'])
    cfa.eval(-1)
    capsys.readouterr()
    for name, m in cfa.metrics.items():
        assert len(m['illum_gain_cfa']) == len(m['illum_gain']) and all(len(g) == 4 and np.isfinite(g).all() for g in m['illum_gain_cfa'])
        assert np.allclose(m['illum_gain'], frame.metrics[name]['illum_gain'], rtol=1e-6, atol=0)       # the total row is the frame's
        for it in range(len(m['psnr'])):
            print(f"[illum driver] {name} round {it}: PSNR(ic) frame {frame.metrics[name]['psnr_ic'][it]:.4f}, cfa {m['psnr_ic'][it]:.4f}")
            assert m['psnr_ic'][it] >= frame.metrics[name]['psnr_ic'][it]
        # --save keeps the uncorrected frame; its sidecar names the last round's gains
        side = json.load(open(os.path.join(cfa.save_dir, name + ".json")))
        assert side['illum_gain'] == m['illum_gain'][-1] and side['illum_gain_cfa'] == m['illum_gain_cfa'][-1]
        saved = np.load(os.path.join(cfa.save_dir, name + ".npy"))
        assert saved.shape == (H, W) and saved.dtype == np.float32

    # the runfile key does the same; the flag overrides it; anything else is refused
    rf2 = _runfile(tmp_path, "any_ic.yml", illum_corr='cfa')
    assert Y.YOND_Full(['-f', rf2, '-m', 'eval', '--synthetic', '1']).illum_corr == 'cfa'
    assert Y.YOND_Full(['-f', rf2, '-m', 'eval', '--synthetic', '1', '--illum-corr', 'frame']).illum_corr == 'frame'
    assert Y.YOND_Full(['-f', rf2, '-m', 'eval', '--synthetic', '1', '--illum-corr', 'off']).illum_corr == 'off'
    rf3 = _runfile(tmp_path, "any_bad.yml", illum_corr='gamma')
    with pytest.raises(YondHipError):
        Y.YOND_Full(['-f', rf3, '-m', 'eval', '--synthetic', '1'])
    with pytest.raises(SystemExit):                                                                      # as it refuses --synth-noise
        YS.YOND_SIDD(['--illum-corr', 'frame'])
