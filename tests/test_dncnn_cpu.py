"""CPU: the DnCNN plug-in's host side -- registry surface, state_dict keys and shapes against the reference's (tests/golden/dncnn.npz),
strict loading, the BatchNorm fold, the refused configurations, the host weight packer of the last layer's kernel (no GPU call)."""
import ctypes

import numpy as np
import pytest
import torch

import dncnn_common as D


def test_registry_exports_the_class():
    from yond_public_amd import archs as A
    assert "DnCNN" in A.__all__ and getattr(A, "DnCNN") is D.DnCNN


@pytest.mark.parametrize("name", ["a", "b"])
def test_state_dict_keys_and_shapes_equal_the_reference(golden, name):
    g = golden("dncnn")
    want = [str(k)[2:] for k in g["keys"] if str(k).startswith(name + ":")]
    net = D.DnCNN(dict(D.CASES[name][0]))
    got = [f"{k}:{'x'.join(map(str, v.shape))}" for k, v in net.state_dict().items()]
    assert got == want                                         # same keys, same order, same shapes (0-d num_batches_tracked: '')
    assert len(want) > 0


@pytest.mark.parametrize("name", ["a", "b"])
def test_strict_load_of_a_reference_shaped_dict(golden, name):
    g = golden("dncnn")
    sd = {}
    for entry in (str(k) for k in g["keys"] if str(k).startswith(name + ":")):
        _, key, shp = entry.split(":")
        shape = tuple(int(v) for v in shp.split("x")) if shp else ()
        sd[key] = torch.zeros(shape, dtype=torch.int64) if key.endswith("num_batches_tracked") else torch.full(shape, 0.25)
    net = D.DnCNN(dict(D.CASES[name][0]))
    res = net.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    # load_weights(by_name=False) (utils/utils.py:160-204): the checkpoint's entries over the model's own state_dict
    state = net.state_dict()
    state.update(sd)
    net.load_state_dict(state)
    assert float(net.dncnn[0].weight.detach()[0, 0, 0, 0]) == 0.25
    with pytest.raises(RuntimeError):
        net.load_state_dict({k: v for k, v in sd.items() if k != "dncnn.0.bias"}, strict=True)


@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_restated_float64_model_equals_the_reference(golden, name):
    """tests/dncnn_common.torch_model64 (what the GPU tests compare modified weights against) and the seeded weights and inputs reproduce
    the reference's float64 outputs (stored to ~1e-14)."""
    g = golden("dncnn")
    args, shape = D.CASES[name]
    sd = D.weights(args, D.case_seed(g["w_seed"], name))
    x = D.case_input(shape, D.case_seed(g["x_seed"], name))
    torch.set_num_threads(8)
    y = D.torch_model64(args, sd, x).numpy()
    assert float(np.abs(y - D.ref64(g, name)).max()) <= 1e-12


def test_batchnorm_fold_equals_torch_eval_mode():
    """escale * z + eshift against torch.nn.BatchNorm2d(eps=1e-4).eval() in float64: each folded vector is the float64 value rounded to
    float32 once, so y differs by at most u (|escale z| + |eshift|), u = 2^-24."""
    from yond_public_amd.dncnn import BN_EPS_REFERENCE, fold_batchnorm
    assert BN_EPS_REFERENCE == 1e-4
    sd = D.weights(D.CASES['a'][0], 5)
    pre = 'dncnn.3.'
    gamma, beta, mean, var = (sd[pre + k] for k in ('weight', 'bias', 'running_mean', 'running_var'))
    assert float(var.min()) >= 0.25 and float(var.max()) <= 4.0 and float(gamma.min()) >= 0.5 and float(mean.abs().max()) > 0.01
    bn = torch.nn.BatchNorm2d(32, eps=1e-4).double().eval()
    bn.load_state_dict({'weight': gamma.double(), 'bias': beta.double(), 'running_mean': mean.double(), 'running_var': var.double(),
                        'num_batches_tracked': torch.tensor(0)})
    z = torch.randn((2, 32, 5, 7), generator=torch.Generator().manual_seed(3), dtype=torch.float64) * 3.0
    with torch.no_grad():
        want = bn(z)
    es, et = fold_batchnorm(gamma, beta, mean, var, 1e-4)
    assert es.dtype == np.float32 and et.dtype == np.float32
    es64, et64 = torch.from_numpy(es.astype(np.float64)), torch.from_numpy(et.astype(np.float64))
    got = z * es64[None, :, None, None] + et64[None, :, None, None]
    bound = 2.0 ** -24 * ((z * es64[None, :, None, None]).abs() + et64.abs()[None, :, None, None]) + 1e-15
    assert bool(((got - want).abs() <= bound).all())
    # a fold with the wrong eps (torch's default 1e-5) or without the mean is outside the bound
    bad = fold_batchnorm(gamma, beta, mean, var, 1e-5)[0].astype(np.float64)
    assert not bool(((z * torch.from_numpy(bad)[None, :, None, None] + et64[None, :, None, None] - want).abs() <= bound).all())


@pytest.mark.parametrize("bad", [dict(in_nc=4, out_nc=3), dict(in_nc=1), dict(out_nc=1), dict(depth=2), dict(nf=48), dict(nf=160), dict(nf=16)])
def test_refused_configurations(bad):
    from yond_public_amd._lib import YondHipError
    with pytest.raises(YondHipError):
        D.DnCNN(D.dn_args(**bad))


def test_bad_precision_and_cpu_tensor_are_refused():
    from yond_public_amd._lib import YondHipError
    with pytest.raises(ValueError):
        D.DnCNN(D.dn_args(precision='bf16'))
    net = D.DnCNN(D.dn_args(depth=3, nf=32)).eval()
    with pytest.raises(YondHipError):
        net(torch.zeros(1, 4, 32, 32))


def test_last_layer_weight_packer_layout_and_argument_checks():
    """yond_pack_conv3x3_out4_weight_f32: OIHW [4][cin][3][3] -> [tap][cin / 4][co][cin % 4]; the entry points check their arguments
    before any launch."""
    from yond_public_amd import _lib
    lib = _lib.load()
    assert lib.yond_abi_version() == 8                       # additive: the version stays
    cin = 48
    w = np.arange(4 * cin * 9, dtype=np.float32).reshape(4, cin, 3, 3)
    dst = np.full(36 * cin, -1.0, np.float32)
    assert lib.yond_pack_conv3x3_out4_weight_f32(w.ctypes.data, cin, dst.ctypes.data) == 0
    d = dst.reshape(9, cin // 4, 4, 4)
    for tap, ci, co in [(0, 0, 0), (8, 47, 3), (4, 21, 2), (5, 6, 1)]:
        assert d[tap, ci // 4, co, ci % 4] == w[co, ci, tap // 3, tap % 3]
    assert sorted(dst.tolist()) == sorted(w.reshape(-1).tolist())
    assert lib.yond_pack_conv3x3_out4_weight_f32(w.ctypes.data, 40, dst.ctypes.data) == -2
    assert lib.yond_pack_conv3x3_out4_weight_f32(w.ctypes.data, 144, dst.ctypes.data) == -2
    assert lib.yond_pack_conv3x3_out4_weight_f32(None, 48, dst.ctypes.data) == -1
    p = ctypes.c_void_p(dst.ctypes.data)                      # (never dereferenced: every call below fails its checks)
    assert lib.yond_conv3x3_out4_f32(None, 64, p, None, None, 1.0, 1, 8, 8, p, None) == -1
    assert lib.yond_conv3x3_out4_f32(p, 64, p, None, None, 0.5, 1, 8, 8, p, None) == -1
    assert lib.yond_conv3x3_out4_f32(p, 64, p, None, None, 1.0, 0, 8, 8, p, None) == -1
    assert lib.yond_conv3x3_out4_f32(p, 24, p, None, None, 1.0, 1, 8, 8, p, None) == -2
    assert lib.yond_conv3x3_out4_f32(p, 256, p, None, None, -1.0, 1, 8, 8, p, None) == -2
