"""CPU: the EstUnet plugin surface (keys, shapes, refusals), the drivers' loading of the runfile's est_* sections, the PGE.npy
per-block table and the configurations refused before any GPU work."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import estnet_common as E  # noqa: E402

from yond_public_amd import archs, estnet, pipeline as P, synthetic as S  # noqa: E402
from yond_public_amd._lib import YondHipError  # noqa: E402
from yond_public_amd.YOND_SIDD import load_estimators  # noqa: E402


def test_exported_by_name():
    assert "EstUnet" in archs.__all__ and getattr(archs, "EstUnet") is archs.EstUnet


def test_keys_and_shapes_are_the_references(golden):
    fx = golden("estnet")
    keys = []
    for name, args in E.MAP_CASES.items():
        keys += [f"{name}:{k}:{'x'.join(map(str, v.shape))}" for k, v in archs.EstUnet(dict(args)).state_dict().items()]
    keys += [f"mean:{k}:{'x'.join(map(str, v.shape))}" for k, v in archs.EstUnet(dict(E.MEAN_ARGS, pge=False)).state_dict().items()]
    assert keys == list(fx["keys"])
    assert any(k.startswith("mean:noiseSTD:") for k in keys)


def test_reference_defaults():
    net = archs.EstUnet({'in_nc': 1})
    assert net.args == dict(out_nc=4, in_nc=1, depth=3, nf=64, nframes=1, res=False, up_mode='transpose', merge_mode='add',
                            use_type='std', pge=True)
    assert net.state_dict()['conv_final.weight'].shape == (4, 64, 1, 1)


@pytest.mark.parametrize("kw,word", [({'up_mode': 'upsample'}, 'upsample'), ({'in_nc': 4}, 'in_nc'), ({'nframes': 2}, 'nframes'),
                                     ({'precision': 'fp16'}, 'fp16'), ({'use_type': 'log'}, 'use_type'), ({'out_nc': 5}, 'out_nc')])
def test_refusals_name_the_setting(kw, word):
    with pytest.raises((YondHipError, ValueError), match=word):
        archs.EstUnet(E.est_args(**kw))


def test_bad_merge_mode_raises_as_reference():
    with pytest.raises(ValueError, match="merging"):
        archs.EstUnet(E.est_args(merge_mode='sum'))


def test_cpu_tensor_and_shape_refused():
    net = archs.EstUnet(E.est_args())
    with pytest.raises(YondHipError, match="ROCm"):
        net(torch.zeros(1, 1, 64, 64))
    with pytest.raises(YondHipError, match="depth"):
        estnet.check_shape(3, 66, 64)                  # the reference raises at the merge for 66 x 64
    estnet.check_shape(3, 64, 64)
    estnet.check_shape(1, 65, 63)


def test_driver_loads_est_sections(tmp_path):
    args = E.est_args(depth=2, nf=32)
    net = archs.EstUnet(dict(args))
    sd = S.procedural_state_dict(net, 5)
    path = tmp_path / "est.pth"
    torch.save(sd, path)
    run = {'est_net': dict(args, weights=str(path)), 'est_self': dict(args, weights=str(tmp_path / "missing.pth"), k=19),
           'arch': {'name': 'GuidedResUnet'}}
    est_args, nets = load_estimators(run, 'cpu')
    assert sorted(est_args) == ['est_net', 'est_self'] and sorted(nets) == ['est_net', 'est_self']
    got = nets['est_net'].state_dict()
    assert all(torch.equal(got[k], sd[k]) for k in sd)
    # missing weights: deterministic estimation weights whose head bias is a plausible (beta1, sqrt(beta2))
    b = nets['est_self'].state_dict()['conv_final.bias']
    assert torch.allclose(b, torch.tensor([4.0 / 959, 6.0 / 959]))
    again = load_estimators(run, 'cpu')[1]['est_self'].state_dict()
    assert all(torch.equal(again[k], v) for k, v in nets['est_self'].state_dict().items())


def test_driver_rejects_unknown_estimator_name():
    with pytest.raises(SystemExit, match="NoSuchNet"):
        load_estimators({'est_net': {'name': 'NoSuchNet'}}, 'cpu')


def test_pge_block_table_squares_the_std_column(tmp_path):
    d = tmp_path / "SIDD_Validation_Raw"
    d.mkdir()
    table = np.random.default_rng(0).uniform(0.001, 0.02, (3, 32, 2))
    np.save(d / "PGE.npy", table)
    reg = P.pge_block_table({'root_dir': str(tmp_path), 'img_id': 1})
    assert reg.shape == (32, 2)
    assert np.array_equal(reg[:, 0], table[1, :, 0]) and np.array_equal(reg[:, 1], table[1, :, 1] ** 2)
    with pytest.raises(YondHipError, match="PGE.npy"):
        P.pge_block_table({'root_dir': None, 'img_id': 1})


def test_pge_blocks_with_iter_refused_before_gpu_work():
    pipe = {'est_type': 'pge', 'full_est': False, 'iter': 'iter', 'full_dn': False, 'bias_corr': 'pre'}
    with pytest.raises(YondHipError, match="once"):
        P.IterDenoise(np.zeros((32, 256, 256), np.float32), None, {'name': 'GuidedResUnet'}, pipe)


def test_ours_needs_section_k():
    with pytest.raises(NotImplementedError, match="est_self"):
        P._section_k({'est_args': {}}, 'est_self')
    assert P._section_k({'est_args': {'est_collab': {'k': 23}}}, 'est_collab') == 23


def test_estimation_weights_are_deterministic():
    net = archs.EstUnet(E.est_args(depth=2, nf=32))
    a = S.estimation_state_dict(net, (0.01, 0.02), seed=3)
    b = S.estimation_state_dict(net, (0.01, 0.02), seed=3)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert torch.equal(a['conv_final.bias'], torch.tensor([0.01, 0.02]))
    assert torch.equal(a['conv_final.weight'], S.procedural_state_dict(net, 3)['conv_final.weight'] * 1e-3)


def test_driver_loads_a_checkpoint_without_every_key(tmp_path):
    """load_weights(by_name=False) starts from the model's own state_dict: a checkpoint without noiseSTD loads; an unknown key raises."""
    args = E.est_args(depth=2, nf=32)
    sd = S.procedural_state_dict(archs.EstUnet(dict(args)), 6)
    del sd['noiseSTD']
    torch.save(sd, tmp_path / "est.pth")
    _, nets = load_estimators({'est_net': dict(args, weights=str(tmp_path / "est.pth"))}, 'cpu')
    got = nets['est_net'].state_dict()
    assert all(torch.equal(got[k], v) for k, v in sd.items()) and 'noiseSTD' in got
    sd['not_a_key'] = torch.zeros(1)
    torch.save(sd, tmp_path / "bad.pth")
    with pytest.raises(RuntimeError, match="not_a_key"):
        load_estimators({'est_net': dict(args, weights=str(tmp_path / "bad.pth"))}, 'cpu')


def test_head_workspace_size_comes_from_the_library():
    from yond_public_amd import _lib
    lib = _lib.load()
    assert lib.yond_est_head_ws_bytes(3, 2) == 3 * 512 * 2 * 8
    assert lib.yond_est_head_ws_bytes(1, 5) == 0
