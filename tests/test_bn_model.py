"""CPU: tests/bn_model.py against torch.nn.BatchNorm2d(C, eps=1e-4, momentum=0.95) + ReLU in float64 train mode (output, the three
buffers, autograd's dx, dgamma, dbeta), and the model of the kernels' arithmetic against the exact model within the derived bounds --
the bounds are checked here, on the CPU, before any kernel is held to them."""
import numpy as np
import pytest
import torch

import bn_model as B


def _torch64(y, dout, gamma, beta, rm, rv, shape):
    """BatchNorm2d + ReLU in float64 train mode on the [N][H][W][C] view of y; returns NHWC-flattened arrays."""
    N, H, W = shape
    C = y.shape[1]
    bn = torch.nn.BatchNorm2d(C, eps=1e-4, momentum=0.95).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma).double())
        bn.bias.copy_(torch.from_numpy(beta).double())
        bn.running_mean.copy_(torch.from_numpy(rm).double())
        bn.running_var.copy_(torch.from_numpy(rv).double())
    x = torch.from_numpy(y).double().reshape(N, H, W, C).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    out = torch.relu(bn(x))
    out.backward(torch.from_numpy(dout).double().reshape(N, H, W, C).permute(0, 3, 1, 2))
    flat = lambda t: t.detach().permute(0, 2, 3, 1).reshape(-1, C).numpy()
    return dict(out=flat(out), dx=flat(x.grad), dgamma=bn.weight.grad.numpy(), dbeta=bn.bias.grad.numpy(), rm=bn.running_mean.numpy(),
                rv=bn.running_var.numpy(), nbt=int(bn.num_batches_tracked))


SHAPES = {'m2': (1, 1, 2), 'ragged': (3, 5, 7), 'constant': (1, 3, 5), 'dead': (1, 4, 6), 'boundary': (1, 3, 4)}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_model_equals_torch_batchnorm_relu_float64(name):
    y, dout, gamma, beta, rm, rv = B.make_case(name, 32)
    ref = _torch64(y, dout, gamma, beta, rm, rv, SHAPES[name])
    fwd = B.exact(y, gamma, beta, rm, rv)
    bwd = B.exact_backward(y, dout, ref['out'] > 0, fwd)
    assert ref['nbt'] == 1
    for got, want in ((fwd['out'], ref['out']), (fwd['rm_new'], ref['rm']), (fwd['rv_new'], ref['rv']), (bwd['dy'], ref['dx']),
                      (bwd['dgamma'], ref['dgamma']), (bwd['dbeta'], ref['dbeta'])):
        scale = max(1.0, float(np.abs(want).max()))
        assert float(np.abs(got - want).max()) <= 1e-11 * scale
    # the model's own mask is torch's (no pre-activation of these cases sits within float64 rounding of zero, except exact zeros)
    assert np.array_equal(fwd['out'] > 0, ref['out'] > 0)
    if name == 'boundary':
        # an output of exactly 0 passes no gradient (torch's ReLU): those elements' g is 0, so their dx is -scale dbeta / M alone
        assert (fwd['out'][2:, 0] == 0).all() and (ref['out'][2:, 0] == 0).all() and (bwd['g'][2:, 0] == 0).all()
        assert np.allclose(ref['dx'][2:, 0], -fwd['scale'][0] * ref['dbeta'][0] / 12, rtol=1e-12, atol=0)


def test_unbiased_factor_at_two_values_per_channel():
    y, dout, gamma, beta, rm, rv = B.make_case('m2', 64)
    fwd = B.exact(y, gamma, beta, rm, rv)
    var_unbiased = y.astype(np.float64).var(0, ddof=1)
    assert np.allclose(fwd['rv_new'], 0.05 * rv.astype(np.float64) + 0.95 * var_unbiased, rtol=1e-12, atol=0)


@pytest.mark.parametrize("C", [32, 96])
@pytest.mark.parametrize("name", B.CASE_NAMES)
def test_kernel_arithmetic_stays_within_the_derived_bounds(name, C):
    """The restated kernel arithmetic (float64 sums, float32 roundings, fma) against the exact model: every output inside its bound,
    with room -- a bound that the arithmetic itself cannot keep would be a wrong derivation."""
    y, dout, gamma, beta, rm, rv = B.make_case(name, C)
    fwd = B.exact(y, gamma, beta, rm, rv)
    k = B.kernel(y, gamma, beta, rm, rv)
    bd = B.bounds(y, gamma, beta, rm, rv, fwd)
    ratios = {n: B.worst_ratio(k['stat'][i], fwd[n], bd[n]) for i, n in enumerate(('mean', 'rstd', 'scale', 'shift'))}
    ratios['out'] = B.worst_ratio(k['out'], fwd['out'], bd['out'])
    ratios['rm_new'] = B.worst_ratio(k['pending'][0], fwd['rm_new'], bd['rm_new'])
    ratios['rv_new'] = B.worst_ratio(k['pending'][1], fwd['rv_new'], bd['rv_new'])
    with np.errstate(invalid='ignore'):
        mask = k['out'] > 0
    bwd = B.exact_backward(y, dout, mask, fwd)
    kb = B.kernel_backward(y, dout, k['stat'])
    bb = B.bounds_backward(y, fwd, bwd)
    for n in ('dbeta', 'dgamma', 'dy'):
        ratios[n] = B.worst_ratio(kb[n], bwd[n], bb[n])
    print(name, C, {n: round(r, 3) for n, r in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios
    if name == 'constant':
        assert k['stat'][1][3] == np.float32(100.0) and fwd['var'][3] == 0
    if name == 'dead':
        assert (kb['dgamma'][1:3] == 0).all() and (kb['dbeta'][1:3] == 0).all() and (k['out'][:, 1:3] == 0).all()
    if name == 'nan':
        bad = np.zeros(C, bool)
        bad[7] = True
        assert np.isnan(k['out'][:, 7]).all() and np.isfinite(k['out'][:, ~bad]).all()
        assert np.isnan(kb['dy'][:, 7]).all() and np.isfinite(kb['dy'][:, ~bad]).all()
        assert np.isfinite(kb['dgamma'][~bad]).all() and np.isfinite(kb['dbeta'][~bad]).all()
