"""Seeded inputs of tests/golden/fbinet_train.npz (tools/gen_golden_fbinet_train.py writes it; tests/test_fbinet_train_model.py and
tests/test_hip_fbinet_train.py read it): the three FBI_Net training cases, their weights and batches regenerated from the seed stored in
the fixture, which taps are live, the PReLUs in forward order, and how tensors are stored.  Imports no reference code."""
import numpy as np
import torch

import fbinet_common as D

#          settings                                                                            Charbonnier loss
CASES = {
    'lin': (D.fbi_args(nf=32, num_of_layers=3), False),                                                    # a x + b, linear
    'sig': (D.fbi_args(nf=32, num_of_layers=3, output_type='sigmoid'), False),                             # sigmoid on a
    'nores': (D.fbi_args(nf=32, num_of_layers=3, res=False, output_channel=1), True),                      # one output, no affine form
}
MOSAIC = (1, 1, 8, 12)
LR = 1e-3
STEPS = 2
MARGIN = 1e-5                     # the smallest |PReLU input| in units of its layer's RMS (the generator's condition on the seed)


def weights(name, seed):
    return D.weights(CASES[name][0], int(seed))


def batch(seed, k):
    """Training batch k (0, 1) as mosaics [1][1][8][12]: (noisy, clean)."""
    g = torch.Generator().manual_seed(int(seed) * 16 + k + 1)
    hr = torch.rand(MOSAIC, generator=g) * 0.8 + 0.05
    lr = (hr + torch.randn(MOSAIC, generator=g) * 0.08).clamp(0, 1)
    return lr, hr


SAMPLE_ABOVE, SAMPLE_N = 600, 576  # (this net has some 50 parameter tensors: a quarter of the DnCNN fixture's sample keeps the file its size)


def sample(a):
    """A tensor as the fixture stores it, by dncnn_train_common.sample's rule: whole up to 600 elements, else 576 of them at a fixed stride."""
    a = np.asarray(a).reshape(-1)
    return a if a.size <= SAMPLE_ABOVE else a[::a.size // SAMPLE_N][:SAMPLE_N]


def flat(tensors, names):
    """{name: array} -> (the tensors' live-tap samples back to back in the order of `names`, [(name, start, stop)]): the fixture holds one
    array per step and kind (a zip member per tensor would cost more than its data)."""
    parts, segs, o = [], [], 0
    for k in names:
        a = np.asarray(tensors[k], np.float64)
        a = sample(a * live_mask(k, a.shape))
        parts.append(a)
        segs.append((k, o, o + a.size))
        o += a.size
    return np.concatenate(parts), segs


def mask_bits(acts, names):
    """{slope name: PReLU input [N][H][W][C]} -> the branches (> 0) of all PReLUs in the order of `names`, np.packbits."""
    return np.packbits(np.concatenate([(np.asarray(acts[k]) > 0).reshape(-1) for k in names]))


def live_mask(key, shape):
    """1 where a parameter's element takes part in the forward: the masked convolutions' live taps, everything of any other tensor."""
    name = key.split('.')[-3] if key.endswith('.conv1.weight') else ''
    if name in D.MASKS:
        return np.broadcast_to(np.asarray(D.MASKS[name], np.float64), shape)
    return np.ones(shape, np.float64)


def prelu_names(args):
    """The slope parameters of the net's PReLUs in forward order (TrainStep.last_acts' keys)."""
    rm = lambda pre: [pre + 'residual_module.activation1.weight', pre + 'residual_module.activation2.weight']
    names = ['new1.activation_new1.weight'] + rm('new1.')
    for i in range(int(args['num_of_layers']) - 1):
        pre = 'new2.' if i == 0 else f'new_{i - 1}.'
        names += [pre + 'activation_new1.weight', pre + 'activation_new2.weight'] + rm(pre)
    return names + ['activation.weight'] + rm('')


def f64(g, key):
    """A stored float64 result: the float32 one plus the float32-rounded difference (as fbinet_common.ref64)."""
    return g[key].astype(np.float64) + g[key.replace('/', '_d64/', 1)].astype(np.float64)
