"""Seeded inputs of tests/golden/dncnn_train.npz (tools/gen_golden_dncnn_train.py writes it, tests/test_hip_dncnn_train.py reads it): the
two DnCNN settings, the weights, the two training batches and the evaluation input, regenerated from the seed stored in the fixture;
and how tensors are sampled and the float64 run is stored.  Imports no reference code."""
import numpy as np
import torch

import dncnn_common as D

VARIANTS = {'bn': D.dn_args(depth=4, nf=32, use_bn=True, res=True), 'nobn': D.dn_args(depth=4, nf=32, use_bn=False, res=True)}
SHAPE = (2, 4, 16, 16)
LR = 1e-3
STEPS = 2
MARGIN = 1e-4                     # the smallest |pre-activation| of every ReLU, in units of that layer's RMS (the generator's condition)
SAMPLE_ABOVE, SAMPLE_N = 2400, 2304


def weights(name, seed):
    return D.weights(VARIANTS[name], int(seed))


def batch(seed, k):
    """Training batch k (0, 1) and the evaluation input (k = 2): (noisy [2][4][16][16], clean)."""
    g = torch.Generator().manual_seed(int(seed) * 16 + k + 1)
    hr = torch.rand(SHAPE, generator=g) * 0.8 + 0.05
    sigma = torch.tensor([0.04, 0.11]).view(-1, 1, 1, 1)
    lr = (hr + torch.randn(SHAPE, generator=g) * sigma).clamp(0, 1)
    return lr, hr


def sample(a):
    """A tensor as the fixture stores it: whole up to 2400 elements, else 2304 of them at a fixed stride."""
    a = np.asarray(a).reshape(-1)
    return a if a.size <= SAMPLE_ABOVE else a[::a.size // SAMPLE_N][:SAMPLE_N]


def relu_indices(name):
    """The indices in `dncnn` whose INPUT is a ReLU's pre-activation (the reference's nn.ReLU modules)."""
    args = VARIANTS[name]
    per = 3 if args['use_bn'] else 2
    return [1] + [2 + per * j + per - 1 for j in range(args['depth'] - 2)]


def f64(g, key):
    """A stored float64 result: the float32 one plus the float32-rounded difference (as dncnn_common.ref64)."""
    return g[key].astype(np.float64) + g[key.replace('/', '_d64/', 1)].astype(np.float64)
