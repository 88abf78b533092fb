"""GPU: the full-frame driver with the robust fit -- `YOND_any --fit ransac --synth-noise 4,6` on synthetic frames, and the
runfile key pipeline.est_fit."""
import os

import numpy as np
import pytest
import yaml

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_driver_fit_ransac(tmp_path, monkeypatch, capsys):
    from yond_public_amd import YOND_full as Y
    from yond_public_amd._lib import YondHipError
    monkeypatch.chdir(tmp_path)
    H, W = 256, 384
    cfg = yaml.load(open(os.path.join(ROOT, "runfiles", "YOND", "ANY_simple+full_pre_grumix.yml")).read(), Loader=yaml.FullLoader)
    for sec in ('dst', 'dst_eval', 'dst_test'):
        cfg[sec].update(root_dir=str(tmp_path / "nowhere"), H=H, W=W)
    rf = tmp_path / "any.yml"
    rf.write_text(yaml.dump(cfg))
    drv = Y.YOND_Full(['-f', str(rf), '-m', 'eval', '--synthetic', '1', '--synth-noise', '4,6', '--fit', 'ransac'])
    assert drv.fit == 'ransac' and drv.pipe['est_fit'] == 'ransac'
    res = drv.eval(-1)
    out = capsys.readouterr().out
    assert "fit ransac: mean |K_est - K| / K" in out
    for red in res.values():
        assert red['count'] == 1 and np.isfinite(red['rel_err_K_iter0']) and np.isfinite(red['rel_err_sigma_iter0'])
    for m in drv.metrics.values():
        assert all(len(e) == 2 and np.isfinite(e).all() for e in m['rel_err']) and len(m['psnr']) >= 1

    # the default names the least-squares fit and gives another estimate on the same frames
    plain = Y.YOND_Full(['-f', str(rf), '-m', 'eval', '--synthetic', '1', '--synth-noise', '4,6'])
    assert plain.fit == 'lsq' and 'est_fit' not in plain.pipe
    res0 = plain.eval(-1)
    assert "fit lsq: mean |K_est - K| / K" in capsys.readouterr().out
    assert any(res0[k]['rel_err_K_iter0'] != res[k]['rel_err_K_iter0'] for k in res)

    # the runfile key does the same; --fit overrides it; anything else is refused
    cfg['pipeline']['est_fit'] = 'ransac'
    rf2 = tmp_path / "any_ransac.yml"
    rf2.write_text(yaml.dump(cfg))
    assert Y.YOND_Full(['-f', str(rf2), '-m', 'eval', '--synthetic', '1']).fit == 'ransac'
    assert Y.YOND_Full(['-f', str(rf2), '-m', 'eval', '--synthetic', '1', '--fit', 'lsq']).fit == 'lsq'
    cfg['pipeline']['est_fit'] = 'huber'
    rf3 = tmp_path / "any_bad.yml"
    rf3.write_text(yaml.dump(cfg))
    with pytest.raises(YondHipError):
        Y.YOND_Full(['-f', str(rf3), '-m', 'eval', '--synthetic', '1'])
