"""GPU: the full-frame driver with the noise-model KLD -- `YOND_any --noise-kld est | K,SIGMA | cam:SPEC` on synthetic frames whose
noise the driver makes itself (`--synth-noise 4,6`), the runfile keys pipeline.noise_kld*, and the refusals.

Frame size.  256 x 384 at ratio 2: in the NumPy model alone (tests/noisekld_model.py on the same clean frame, three seeds, both ratios of
the runfile) the true model (4, 6) gives a KLD of 1.0 - 1.6 times its floor (5e-4 .. 9e-4 against 3e-4 .. 8e-4) and the wrong one
(8, 6) 70 - 180 times (5.7e-2 .. 6.5e-2): the two asserted inequalities, 10 times the floor on either side, hold with a wide margin.
"""
import os
import zlib

import numpy as np
import pytest
import yaml

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 256, 384
RATIO = 2
CAM = 'code=p,K=4,sigGs=6'


def _runfile(tmp_path, name, **pipeline):
    cfg = yaml.load(open(os.path.join(ROOT, "runfiles", "YOND", "ANY_simple+full_pre_grumix.yml")).read(), Loader=yaml.FullLoader)
    for sec in ('dst', 'dst_eval', 'dst_test'):
        cfg[sec].update(root_dir=str(tmp_path / "nowhere"), H=H, W=W, ratio_list=[RATIO])
    cfg['pipeline'].update(pipeline)
    rf = tmp_path / name
    rf.write_text(yaml.dump(cfg))
    return str(rf)


def test_driver_noise_kld(tmp_path, monkeypatch, capsys):
    import torch
    from yond_public_amd import YOND_full as Y
    from yond_public_amd import YOND_SIDD as YS
    from yond_public_amd import camnoise as CN
    from yond_public_amd import noisekld as NK
    from yond_public_amd import pgnoise as PG
    monkeypatch.chdir(tmp_path)
    rf = _runfile(tmp_path, "any.yml")
    base = ['-f', rf, '-m', 'eval', '--synthetic', '1', '--synth-noise', '4,6']
    n_it = 2
    want = {'count', 'psnr_last', 'ssim_last'} | {f'{k}_iter{it}' for it in range(n_it) for k in ('psnr', 'ssim', 'rel_err_K', 'rel_err_sigma')}
    plain_keys = {'psnr', 'ssim', 'reg', 'true', 'rel_err'}
    kld_keys = {'kld', 'kld_cfa', 'kld_bands', 'kld_floor'}

    # the switch off: the keys and the log of today
    plain = Y.YOND_Full(base)
    assert plain.noise_kld is None and not any(k.startswith('noise_kld') for k in plain.pipe)
    res0 = plain.eval(-1)
    out0 = capsys.readouterr().out
    assert "KLD" not in out0 and "kld" not in out0 and "Noise model" not in out0
    assert res0 and all(set(red) == want for red in res0.values())
    assert plain.metrics and all(set(m) == plain_keys for m in plain.metrics.values())

    # --noise-kld est with four bands
    est = Y.YOND_Full(base + ['--noise-kld', 'est', '--kld-bands', '4'])
    assert est.noise_kld == ('est',) and est.kld_bands == 4 and est.kld_range == 0.1 and not any(k.startswith('noise_kld') for k in est.pipe)
    res = est.eval(-1)
    out = capsys.readouterr().out
    assert any("KLD=" in line and "(cfa " in line and "(bands " in line and "KLD floor=" in line for line in out.splitlines())
    assert any("mean KLD=" in line and "mean KLD floor=" in line for line in out.splitlines())
    assert set(est.metrics) == set(plain.metrics)
    for name, m in est.metrics.items():
        assert set(m) == plain_keys | kld_keys
        assert len(m['kld_cfa']) == 4 and len(m['kld_bands']) == 4
        assert np.isfinite([m['kld'], m['kld_floor']] + m['kld_cfa'] + m['kld_bands']).all() and m['kld'] >= 0 and m['kld_floor'] > 0
        # the plain metrics stay where they are (two runs of the pipeline: equal up to the order of the estimator's atomic sums)
        assert np.allclose(m['psnr'], plain.metrics[name]['psnr'], rtol=1e-6, atol=0) and m['true'] == plain.metrics[name]['true']
        print(f"[noisekld driver] {name} est: KLD {m['kld']:.3e}, floor {m['kld_floor']:.3e}, cfa {m['kld_cfa']}, bands {m['kld_bands']}")
    for label, red in res.items():
        assert set(red) == want | {'kld', 'kld_floor'}
        assert all(np.isclose(red[k], res0[label][k], rtol=1e-6, atol=0) for k in want)
        assert np.isclose(red['kld'], np.mean([m['kld'] for m in est.metrics.values()]), rtol=0, atol=1e-15)

    # the true level sits at its own floor, a wrong gain far above it
    kld = {}
    for level in ('4,6', '8,6'):
        drv = Y.YOND_Full(base + ['--noise-kld', level])
        assert drv.noise_kld == ('pg',) + tuple(float(v) for v in level.split(','))
        drv.eval(-1)
        capsys.readouterr()
        for name, m in drv.metrics.items():
            assert len(m['kld_bands']) == 1 and m['kld_bands'][0] == m['kld']          # no bands: the one band is the frame
            print(f"[noisekld driver] {name} model {level}: KLD {m['kld']:.3e}, floor {m['kld_floor']:.3e}")
            kld[level] = m
    assert kld['4,6']['kld'] < 10 * kld['4,6']['kld_floor']
    assert kld['8,6']['kld'] > 10 * kld['8,6']['kld_floor']

    # cam: runs, and agrees with the library called by hand on the frame the driver made
    rf2 = _runfile(tmp_path, "any_kld.yml", noise_kld='cam:' + CAM, noise_kld_range=0.2, noise_kld_bands=2)
    cam = Y.YOND_Full(['-f', rf2, '-m', 'eval', '--synthetic', '1', '--synth-noise', '4,6'])
    assert cam.noise_kld[0] == 'cam' and cam.kld_range == 0.2 and cam.kld_bands == 2
    cam.eval(-1)
    capsys.readouterr()
    frames = Y.SyntheticFrames(1, H, W, clean_only=True)
    frames.change_eval_ratio(ratio=RATIO)
    item = frames[0]
    m = cam.metrics[item['name']]
    wp, bl = float(cam.dst.get('wp', 1023)), float(cam.dst.get('bl', 64))
    clean = torch.from_numpy(item['hr']).cuda()
    noisy = PG.add_pg_noise(clean, 4.0, 6.0, wp - bl, zlib.crc32(item['name'].encode()), [0], exposure=1.0 / RATIO)
    edges, spec = NK.kld_edges(0.2), CN.camera_noise_arg(CAM)
    q = [NK.residual_hist(CN.add_camera_noise(clean, dict(spec, wp=wp, bl=bl), spec['code'], wp - bl, zlib.crc32((item['name'] + tag).encode()), [0],
                                              layout=CN.LAYOUT_BAYER, ratio=RATIO, mfm=spec['mfm'], clip=spec['clip']), clean, edges, 2)
         for tag in ('/kld0', '/kld1')]
    by_hand = NK.kld_report(NK.residual_hist(noisy, clean, edges, 2), q[0], clean.numel())
    assert m['kld'] == by_hand['kld'] and m['kld_cfa'] == by_hand['kld_cfa'] and m['kld_bands'] == by_hand['kld_bands']
    assert m['kld_floor'] == NK.kld_report(q[1], q[0], clean.numel())['kld']
    # code p with Gaussian read noise IS the Poisson-Gaussian model (bit for bit, include/yond_hip.h I3): the fused launch gives its counts
    fused = NK.pg_model_hist(clean, 4.0, 6.0, wp - bl, zlib.crc32((item['name'] + '/kld0').encode()), edges, 2, exposure=1.0 / RATIO)
    assert bool((fused == q[0]).all())
    assert m['kld'] < 10 * m['kld_floor']

    # the flags override the runfile; YOND_SIDD refuses the switch as it refuses --synth-noise
    over = Y.YOND_Full(['-f', rf2, '-m', 'eval', '--synthetic', '1', '--noise-kld', 'est', '--kld-range', '0.05', '--kld-bands', '0'])
    assert over.noise_kld == ('est',) and over.kld_range == 0.05 and over.kld_bands == 0
    with pytest.raises(SystemExit):
        YS.YOND_SIDD(['--noise-kld', 'est'])
    with pytest.raises(SystemExit):
        Y.YOND_Full(base + ['--noise-kld', 'gamma'])
