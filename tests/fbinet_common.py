"""Seeded inputs of tests/golden/fbinet.npz (tools/gen_golden_fbinet.py writes it; tests/test_fbinet_cpu.py, tests/test_hip_fbinet.py and
tests/test_hip_fbinet_kernels.py read it): the FBI_Net settings of every case, the weights and the inputs, regenerated from the seeds
stored in the fixture, and the network restated in float64.  Imports no reference code."""
import numpy as np
import torch

from yond_public_amd.archs import FBI_Net
from yond_public_amd.synthetic import denoising_state_dict, procedural_state_dict, synth_noisy


def fbi_args(**kw):
    a = dict(name='FBI_Net', channel=1, output_channel=2, nf=64, mul=1, num_of_layers=17, case='FBI_Net', output_type='linear',
             sigmoid_value=0.1, res=True)
    a.update(kw)
    return a


#         settings                                                                        input [N][1][H][W]
CASES = {
    'a': (fbi_args(nf=32, num_of_layers=4), (2, 1, 24, 40)),                                                  # batch, both tap sets once
    'b': (fbi_args(nf=64, num_of_layers=5, res=False, output_channel=1), (1, 1, 32, 32)),                     # no affine output
    'c': (fbi_args(nf=64, num_of_layers=17, output_type='sigmoid'), (1, 1, 64, 96)),                          # the shipped depth, sigmoid
    'd': (fbi_args(nf=32, num_of_layers=3), (1, 1, 6, 10)),                                                   # smaller than the halo
    'e': (fbi_args(nf=64, num_of_layers=4), (3, 1, 38, 50)),                                                  # no tile size divides it
}
# dn_vst: the reference's VST_Denoiser(denoiser='fbi') with net (a) and weakly denoising weights on a Poisson-Gaussian Bayer frame
VST_HW, VST_K, VST_SIGMA, VST_IDX, VST_EPS = (96, 128), 4.0, 6.0, 61, 0.1

MASKS = {'new1': [[1, 1, 1], [1, 0, 1], [1, 1, 1]],
         'new2': [[0, 1, 0, 1, 0], [1, 0, 0, 0, 1], [0, 0, 1, 0, 0], [1, 0, 0, 0, 1], [0, 1, 0, 1, 0]],
         'new3': [[1, 0, 1], [0, 1, 0], [1, 0, 1]]}


def case_seed(base, name):
    return int(base) + 'abcde'.index(name)


def weights(args, seed):
    """The project's per-key seeded filler (fan-in over the live taps; PReLU slopes uniform in [-0.1, 0.4])."""
    return procedural_state_dict(FBI_Net(dict(args)), seed)


def vst_weights(args, seed):
    return denoising_state_dict(FBI_Net(dict(args)), seed, eps=VST_EPS)


def case_input(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(int(seed))) * 0.9


def vst_frame():
    return synth_noisy(VST_HW[0], VST_HW[1], VST_K, VST_SIGMA, VST_IDX)[0]


def vst_params():
    return {'wp': 1023, 'bl': 64, 'ratio': 1, 'scale': 959.0, 'gain': np.float64(VST_K), 'sigma': np.float64(VST_SIGMA)}


def build(args, sd, device):
    net = FBI_Net(dict(args))
    net.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return net.to(device).eval()


def prelu64(x, s):
    """PReLU on NCHW float64 with a [C] (or [1]) slope."""
    return torch.where(x > 0, x, x * s.reshape(1, -1, 1, 1))


def rm64(sd, pre, v):
    """The residual module `pre`residual_module (archs/comp.py:303-322)."""
    import torch.nn.functional as F
    r = pre + 'residual_module.'
    h = prelu64(F.conv2d(v, sd[r + 'conv1_1by1.weight'], sd[r + 'conv1_1by1.bias']), sd[r + 'activation1.weight'])
    return prelu64((v + F.conv2d(h, sd[r + 'conv2_1by1.weight'], sd[r + 'conv2_1by1.bias'])) / 2.0, sd[r + 'activation2.weight'])


def torch_model64(args, sd, x):
    """The network restated with torch.nn.functional in float64: x [N][1][H][W] -> [N][1][H][W] float64."""
    import torch.nn.functional as F
    sd = {k: torch.as_tensor(v).double() for k, v in sd.items()}
    m = {k: torch.tensor(v, dtype=torch.float64) for k, v in MASKS.items()}
    L = int(args['num_of_layers'])
    x = x.double()
    n = prelu64(F.conv2d(x, sd['new1.new1.conv1.weight'] * m['new1'], sd['new1.new1.conv1.bias'], padding=1), sd['new1.activation_new1.weight'])
    o = rm64(sd, 'new1.', n)
    total = o
    for i in range(L - 1):
        pre, conv, pad, dil = ('new2.', 'new2', 2, 1) if i == 0 else (f'new_{i - 1}.', 'new3', 3, 3)
        n = prelu64(F.conv2d(n, sd[f'{pre}{conv}.conv1.weight'] * m[conv], sd[f'{pre}{conv}.conv1.bias'], padding=pad, dilation=dil),
                    sd[pre + 'activation_new1.weight'])
        o = rm64(sd, pre, prelu64((n + o) / 2.0, sd[pre + 'activation_new2.weight']))
        total = total + o
    f = rm64(sd, '', prelu64(total / L, sd['activation.weight']))
    y = F.conv2d(f, sd['output_layer.weight'], sd['output_layer.bias'])
    if args['output_type'] == 'sigmoid':
        y = torch.cat([float(args['sigmoid_value']) * torch.sigmoid(y[:, :1]), y[:, 1:]], dim=1)
    return y[:, :1] * x + y[:, 1:] if args['res'] else y


def ref64(g, name):
    """The float64 reference output of a case: stored as the float32 output plus the float32-rounded difference to it."""
    return g[f"y32_{name}"].astype(np.float64) + g[f"d64_{name}"].astype(np.float64)


def to_packed(x):
    """[N][1][H][W] mosaic -> packed [N][H/2][W/2][4]: element 2 (y & 1) + (x & 1) of the packed pixel (y / 2, x / 2)."""
    N, _, H, W = x.shape
    return x.reshape(N, H // 2, 2, W // 2, 2).permute(0, 1, 3, 2, 4).reshape(N, H // 2, W // 2, 4).contiguous()


def from_packed(x4):
    N, h, w, _ = x4.shape
    return x4.reshape(N, h, w, 2, 2).permute(0, 1, 3, 2, 4).reshape(N, 1, 2 * h, 2 * w).contiguous()
