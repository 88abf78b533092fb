"""CPU: the FBI_Net plug-in's host side -- registry surface, state_dict keys and shapes against the reference's (tests/golden/fbinet.npz),
strict loading, the refused configurations, the runfile, the restated float64 model against the reference's float64 outputs, the
blind-spot property on that model, the synthetic weights, and the entries' argument checks and host weight packers (no GPU call)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fbinet_common as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_registry_exports_the_class():
    from yond_public_amd import archs as A
    assert "FBI_Net" in A.__all__ and getattr(A, "FBI_Net") is D.FBI_Net


@pytest.mark.parametrize("name", ["a", "c"])
def test_state_dict_keys_and_shapes_equal_the_reference(golden, name):
    g = golden("fbinet")
    want = [str(k)[2:] for k in g["keys"] if str(k).startswith(name + ":")]
    net = D.FBI_Net(dict(D.CASES[name][0]))
    got = [f"{k}:{'x'.join(map(str, v.shape))}" for k, v in net.state_dict().items()]
    assert got == want                                         # same keys, same order, same shapes
    if name == "c":
        assert len(want) == 178                                # nf 64, num_of_layers 17
        assert "new1.new1.conv1.weight:64x1x3x3" in got and "new1.activation_new1.weight:1" in got
        assert "new2.new2.conv1.weight:64x64x5x5" in got and "new_14.new3.conv1.weight:64x64x3x3" in got
        assert not any("mask" in k for k in got)


@pytest.mark.parametrize("name", ["a", "c"])
def test_strict_load_of_a_reference_shaped_dict(golden, name):
    g = golden("fbinet")
    sd = {}
    for entry in (str(k) for k in g["keys"] if str(k).startswith(name + ":")):
        _, key, shp = entry.split(":")
        sd[key] = torch.full(tuple(int(v) for v in shp.split("x")), 0.25)
    net = D.FBI_Net(dict(D.CASES[name][0]))
    res = net.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    # load_weights(by_name=False) (utils/utils.py:160-204): the checkpoint's entries over the model's own state_dict, in order
    state = net.state_dict()
    for (k_model, _), (_, v) in zip(list(state.items()), sd.items()):
        state[k_model] = v
    net.load_state_dict(state)
    assert float(net.new1.new1.conv1.weight.detach()[0, 0, 1, 1]) == 0.25      # the weights stay unmasked in the module
    with pytest.raises(RuntimeError):
        net.load_state_dict({k: v for k, v in sd.items() if k != "activation.weight"}, strict=True)


@pytest.mark.parametrize("bad, word", [(dict(case='case3'), 'case'), (dict(channel=4), 'channel'), (dict(res=True, output_channel=1), 'output_channel'),
                                       (dict(res=False, output_channel=2), 'output_channel'), (dict(mul=2), 'mul'), (dict(nf=48), 'nf'),
                                       (dict(nf=128), 'nf'), (dict(num_of_layers=2), 'num_of_layers'), (dict(precision='fp32'), 'precision'),
                                       (dict(precision='fp16'), 'precision'), (dict(output_type='tanh'), 'output_type')])
def test_refused_configurations_name_their_setting(bad, word):
    from yond_public_amd._lib import YondHipError
    with pytest.raises(YondHipError, match=word):
        D.FBI_Net(D.fbi_args(**bad))
    if word == 'precision':
        with pytest.raises(YondHipError, match="not built"):
            D.FBI_Net(D.fbi_args(**bad))


def test_missing_key_and_cpu_tensor_are_refused():
    from yond_public_amd._lib import YondHipError
    args = D.fbi_args()
    del args['mul']
    with pytest.raises(YondHipError, match="mul"):
        D.FBI_Net(args)
    net = D.FBI_Net(D.fbi_args(nf=32, num_of_layers=3, precision='fp32-mfma')).eval()
    assert net.precision == 'fp32-mfma'
    with pytest.raises(YondHipError):
        net(torch.zeros(1, 1, 8, 8))


def test_runfile_parses_to_the_arch_dict():
    import yaml
    cfg = yaml.load(open(os.path.join(ROOT, "runfiles", "YOND", "ANY_simple+full_pre_fbi.yml")).read(), Loader=yaml.FullLoader)
    assert cfg['arch'] == dict(name='FBI_Net', channel=1, output_channel=2, nf=64, mul=1, num_of_layers=17, case='FBI_Net',
                               output_type='linear', sigmoid_value=0.1, res=True)
    assert cfg['pipeline']['denoiser_type'] == 'fbi' and cfg['pipeline']['full_dn'] is True
    D.FBI_Net(cfg['arch'])
    from yond_public_amd import pipeline as P
    assert P.denoiser_of(cfg['pipeline']) == 'fbi' and P.denoiser_of({'denoiser_type': 'unetn'}) is None and P.denoiser_of({}) is None
    assert not P.stream_applies(cfg['pipeline']) and P.stream_applies(dict(cfg['pipeline'], denoiser_type='unetn'))


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_restated_float64_model_equals_the_reference(golden, name):
    """tests/fbinet_common.torch_model64 (what the GPU kernel tests lean on) and the seeded weights and inputs reproduce the reference's
    float64 outputs to 1e-9 relative."""
    g = golden("fbinet")
    args, shape = D.CASES[name]
    sd = D.weights(args, D.case_seed(g["w_seed"], name))
    x = D.case_input(shape, D.case_seed(g["x_seed"], name))
    torch.set_num_threads(8)
    y = D.torch_model64(args, sd, x).numpy()
    want = D.ref64(g, name)
    assert y.shape == want.shape
    assert float(np.abs(y - want).max()) <= 1e-9 * float(np.abs(want).max())


def test_blind_spot_property_of_the_float64_model():
    """With res False the output at a pixel does not depend on the input at that pixel: adding 0.5 there leaves it unchanged (exactly:
    no masked product enters the sum) and changes others."""
    args = D.fbi_args(nf=32, num_of_layers=5, res=False, output_channel=1)
    sd = D.weights(args, 11)
    x = D.case_input((1, 1, 20, 24), 12)
    y0 = D.torch_model64(args, sd, x)
    for (py, px) in [(0, 0), (19, 23), (7, 8), (10, 13)]:
        x1 = x.clone()
        x1[0, 0, py, px] += 0.5
        y1 = D.torch_model64(args, sd, x1)
        assert float((y1 - y0)[0, 0, py, px].abs()) <= 1e-15
        assert int(((y1 - y0).abs() > 1e-9).sum()) > 10


def test_procedural_weights_of_fbinet():
    """PReLU slopes uniform in [-0.1, 0.4] (both signs present), masked convolutions scaled by their live fan-in."""
    args = D.fbi_args()
    sd = D.weights(args, 3)
    slopes = torch.cat([v.reshape(-1) for k, v in sd.items() if 'activation' in k])
    assert float(slopes.min()) >= -0.1 and float(slopes.max()) <= 0.4 and float(slopes.min()) < -0.05 and float(slopes.max()) > 0.35
    assert sd['new1.activation_new1.weight'].shape == (1,)
    for key, live in (('new2.new2.conv1.weight', 9), ('new_3.new3.conv1.weight', 5)):
        assert abs(float(sd[key].std()) * np.sqrt(64 * live) - 1.0) < 0.05
    assert abs(float(sd['new1.new1.conv1.weight'].std()) * np.sqrt(8) - 1.0) < 0.15


@pytest.mark.parametrize("res", [True, False])
def test_denoising_weights_average_the_eight_neighbours(res):
    """synthetic.denoising_state_dict: out = x / 2 + mean8 / 2 (res) or mean8, up to the eps-sized rest -- on the float64 model."""
    import torch.nn.functional as F
    from yond_public_amd.synthetic import denoising_state_dict
    args = D.fbi_args(nf=32, num_of_layers=6, res=res, output_channel=2 if res else 1)
    eps = 1e-3
    sd = denoising_state_dict(D.FBI_Net(dict(args)), 0, eps=eps)
    x = (D.case_input((1, 1, 16, 20), 5) + 0.05).double()
    y = D.torch_model64(args, sd, x)
    k = torch.ones(1, 1, 3, 3, dtype=torch.float64) / 8.0
    k[0, 0, 1, 1] = 0.0
    mean8 = F.conv2d(x, k, padding=1)
    want = x / 2 + mean8 / 2 if res else mean8
    assert float((y - want).abs().max()) <= 0.02
    assert float((y - want).abs().max()) > 0.0


def test_weight_packers_and_argument_checks():
    """The host packers' layouts (only live taps are read) and every entry's refusal of NULL pointers and of shapes it does not take --
    before any launch."""
    from yond_public_amd import _lib
    lib = _lib.load()
    assert lib.yond_abi_version() == 8                       # additive: the version stays
    assert lib.yond_fbi_taps(0) == 9 and lib.yond_fbi_taps(1) == 5 and lib.yond_fbi_taps(2) == -1
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.yond_fbi_tile(ctypes.byref(th), ctypes.byref(tw)) == 0 and th.value >= 1 and tw.value >= 1
    nf = 64
    live = {0: [(0, 1), (0, 3), (1, 0), (1, 4), (2, 2), (3, 0), (3, 4), (4, 1), (4, 3)], 1: [(0, 0), (0, 2), (1, 1), (2, 0), (2, 2)]}
    for tset, k in ((0, 5), (1, 3)):
        w = np.arange(nf * nf * k * k, dtype=np.float32).reshape(nf, nf, k, k)
        dst = np.full(len(live[tset]) * nf * nf, -1.0, np.float32)
        assert lib.yond_pack_fbi_tap_weight_f32(w.ctypes.data, nf, tset, dst.ctypes.data) == 0
        want = sorted(float(w[co, ci, r, c]) for co in range(nf) for ci in range(nf) for (r, c) in live[tset])
        assert sorted(dst.tolist()) == want                  # exactly the live taps, each once
        d = dst.reshape(nf // 16, len(live[tset]), 2, nf // 32, 64, 4)
        for chunk, t, q, ct, lane, e in [(0, 0, 0, 0, 0, 0), (3, len(live[tset]) - 1, 1, 1, 63, 3), (2, 2, 1, 0, 37, 2)]:
            r, c = live[tset][t]
            assert d[chunk, t, q, ct, lane, e] == w[ct * 32 + (lane & 31), chunk * 16 + q * 8 + (lane >> 5) * 4 + e, r, c]
    w = np.arange(nf * nf, dtype=np.float32).reshape(nf, nf)
    dst = np.full(nf * nf, -1.0, np.float32)
    assert lib.yond_pack_fbi_rm_weight_f32(w.ctypes.data, nf, dst.ctypes.data) == 0
    d = dst.reshape(2, 2, 4, 64, 4)
    for cot, ct, g_, lane, e in [(0, 0, 0, 0, 0), (1, 0, 3, 45, 2), (1, 1, 2, 63, 3)]:
        assert d[cot, ct, g_, lane, e] == w[cot * 32 + (lane & 31), ct * 32 + 8 * g_ + 4 * (lane >> 5) + e]
    w = np.arange(nf * 9, dtype=np.float32).reshape(nf, 1, 3, 3)
    dst = np.full(8 * nf, -1.0, np.float32)
    assert lib.yond_pack_fbi_first_weight_f32(w.ctypes.data, nf, dst.ctypes.data) == 0
    assert dst.reshape(8, nf)[4, 7] == w[7, 0, 1, 2] and not np.isin(w[:, 0, 1, 1], dst).any()
    p = ctypes.c_void_p(dst.ctypes.data)                      # (never dereferenced: every call below fails its checks)
    q = ctypes.c_void_p(w.ctypes.data)
    assert lib.yond_pack_fbi_tap_weight_f32(p, 48, 0, p) == -1 and lib.yond_pack_fbi_tap_weight_f32(p, 64, 2, p) == -1
    assert lib.yond_pack_fbi_rm_weight_f32(None, 64, p) == -1 and lib.yond_pack_fbi_first_weight_f32(p, 16, p) == -1
    assert lib.yond_fbi_first_f32(None, 1, 4, 4, 64, p, p, p, p, None) == -1
    assert lib.yond_fbi_first_f32(p, 1, 4, 4, 48, p, p, p, p, None) == -1
    assert lib.yond_fbi_first_f32(p, 1, 0, 4, 64, p, p, p, p, None) == -1
    assert lib.yond_fbi_tapconv_f32(p, q, 0, 64, p, p, p, p, 1, 8, 8, None, q, None) == -1
    assert lib.yond_fbi_tapconv_f32(p, q, 2, 64, p, p, p, p, 1, 8, 8, q, q, None) == -1
    assert lib.yond_fbi_tapconv_f32(p, q, 1, 96, p, p, p, p, 1, 8, 8, q, q, None) == -1
    assert lib.yond_fbi_tapconv_f32(p, q, 1, 64, p, p, p, p, 1, 0, 8, q, q, None) == -1
    assert lib.yond_fbi_tapconv_f32(p, q, 1, 64, p, p, p, p, 1, 8, 8, p, q, None) == -1       # n_out == n_in
    assert lib.yond_fbi_rm_f32(None, 64, p, p, p, p, p, p, None, 0, 16, q, None, 0, None) == -1
    assert lib.yond_fbi_rm_f32(p, 64, p, p, p, p, p, p, None, 0, 0, q, None, 0, None) == -1
    assert lib.yond_fbi_rm_f32(p, 64, p, p, p, p, p, p, None, 0, 16, q, None, 2, None) == -1   # accumulate without a sum
    assert lib.yond_fbi_rm_f32(p, 64, p, p, p, p, p, p, p, 0, 16, q, None, 0, None) == -1      # prologue without its divisor
    assert lib.yond_fbi_rm_f32(p, 40, p, p, p, p, p, p, None, 0, 16, q, None, 0, None) == -1
    assert lib.yond_fbi_out_f32(p, 64, p, p, 2, 0, 0.1, None, 1, 4, 4, q, None) == -1          # a x + b without x
    assert lib.yond_fbi_out_f32(p, 64, p, p, 3, 0, 0.1, p, 1, 4, 4, q, None) == -1
    assert lib.yond_fbi_out_f32(p, 64, p, p, 1, 0, 0.1, None, 1, 4, 0, q, None) == -1
    assert lib.yond_vst_minmax_f32(None, 1, 8, 8, 959.0, 4.0, 6.0, None, None, 0, 0, p, None) == -1
    assert lib.yond_vst_minmax_f32(p, 1, 7, 8, 959.0, 4.0, 6.0, None, None, 0, 0, p, None) == -1    # odd size
    assert lib.yond_vst_minmax_f32(p, 1, 8, 9, 959.0, 4.0, 6.0, None, None, 0, 0, p, None) == -1
    assert lib.yond_vst_minmax_f32(p, 0, 8, 8, 959.0, 4.0, 6.0, None, None, 0, 0, p, None) == -1
    assert lib.yond_vst_minmax_f32(p, 1, 8, 8, 959.0, 0.0, 6.0, None, None, 0, 0, p, None) == -1
    assert lib.yond_vst_minmax_f32(p, 1, 8, 8, 959.0, 4.0, 6.0, None, None, 5, 0, p, None) == -1    # knots announced, none given
