"""Seeded inputs of tests/golden/estnet.npz (tools/gen_golden_estnet.py writes it; tests/test_*estnet*.py read it): the EstUnet
settings of every case, the weights and the frames, regenerated from the seeds stored in the fixture.  Imports no reference code."""
import numpy as np
import torch

from yond_public_amd.archs import EstUnet
from yond_public_amd.synthetic import procedural_state_dict, estimation_state_dict, synth_noisy


def est_args(**kw):
    a = dict(name='EstUnet', in_nc=1, out_nc=2, nframes=1, depth=3, nf=64, res=False, up_mode='transpose', merge_mode='add',
             use_type='std', pge=True)
    a.update(kw)
    return a


# (a) maps, N = 2, 64 x 96
MAP_CASES = {
    'add_std_d3_nf64': est_args(merge_mode='add', use_type='std', depth=3, nf=64, out_nc=4, pge=False),
    'concat_var_d2_nf32': est_args(merge_mode='concat', use_type='var', depth=2, nf=32, out_nc=2, pge=False),
    'd1_nf32': est_args(depth=1, nf=32, out_nc=3, pge=False),
    'd4_nf32': est_args(depth=4, nf=32, out_nc=2, pge=False),
}
MAP_SHAPE = (2, 64, 96)
# (b) means of the default network (depth 3, nf 64, 'add', 'std', out_nc 2)
MEAN_CASES = {'sidd32': (32, 256, 256), 'cat': (1, 256, 8192), 'frame12mp': (1, 3000, 4000)}
MEAN_ARGS = est_args()


# (c), (d) IterDenoise with est_type 'pge' + est_net (and the PGE.npy table) and 'ours' -- the denoiser is GuidedResUnet nf 8 with
# yond_oracle.denoising_state_dict(GRU8, ITER_DN_SEED) (round 2 runs); frames synth_noisy(..., K, sigma, idx)
GRU8 = dict(name='GuidedResUnet', in_nc=4, out_nc=4, nf=8, nframes=1, res=True, norm=True, guided=True)
ITER_DN_SEED = 73
ITER_BASE = {'data_type': 'SIDD', 'full_est': True, 'k': 29, 'vst_type': 'exact', 'bias_corr': 'pre', 'denoiser_type': 'gru32n',
             'iter': 'iter', 'max_iter': 1, 'clip': False, 'full_dn': False}
#        name          est_type  frame (H, W)   full_dn full_est iter    source  K    sigma idx
ITER_CASES = [
    # (est_type exactly 'pge' with full_est and block-wise denoising raises in the reference -- :399-400 index the frame's [2]
    #  estimate per block -- so the SIDD stack case takes 'pge+full', as the shipped runfiles name 'simple+full')
    ('sidd_iter',      'pge+full', (256, 8192), False, True, 'iter', 'net', 4.0, 6.0, 31),
    ('frame_iter',     'pge',  (3000, 4096), True,  True,  'iter', 'net',   2.0, 20.0, 32),
    ('blocks_net',     'pge',  (256, 8192),  False, False, 'once', 'net',   2.0, 20.0, 33),
    ('blocks_table',   'pge',  (256, 8192),  False, False, 'once', 'table', 4.0, 6.0, 34),
    ('ours',           'ours', (256, 8192),  False, True,  'iter', None,    2.0, 20.0, 35),
]
OURS_K = {'est_self': 19, 'est_collab': 23}
ITER_EST_SEED = 41


def iter_pipe(case):
    name, est_type, hw, full_dn, full_est, it, src, K, s, idx = case
    return dict(ITER_BASE, est_type=est_type, full_dn=full_dn, full_est=full_est, iter=it)


def iter_frame(case):
    """(noisy frame [H][W], the est net's true (beta1, sqrt(beta2)))."""
    name, est_type, (H, W), full_dn, full_est, it, src, K, s, idx = case
    noisy, _ = synth_noisy(H, W, K, s, idx)
    return noisy, (K / 959.0, s / 959.0)


def iter_full_frame(case):
    """The separate frame of round 1's self estimate for 'ours' (lr_full / lr_path_full, YOND_SIDD.py:344-345)."""
    name, est_type, hw, full_dn, full_est, it, src, K, s, idx = case
    return synth_noisy(512, 1024, K, s, idx + 100)[0]


def pge_table(case):
    """The PGE.npy stand-in of the table case: [1][32][2] (beta1, sqrt(beta2)) around the frame's true values."""
    name, est_type, hw, full_dn, full_est, it, src, K, s, idx = case
    rng = np.random.default_rng(idx)
    base = np.array([K / 959.0, s / 959.0])
    return (base * rng.uniform(0.8, 1.25, (1, 32, 2))).astype(np.float64)


def iter_crops(dn):
    """What the fixture keeps of one output: a corner, a strip across the middle (a block seam for 256 x 8192) and a strided sample."""
    dn = np.asarray(dn, np.float32)
    H, W = dn.shape
    return (dn[:32, :128], dn[H // 2 - 16:H // 2 + 16, W // 2 - 32:W // 2 + 32], dn[5::H // 16, 3::64])


def weights(args, seed):
    return procedural_state_dict(EstUnet(dict(args)), seed)


def estimation_weights(args, seed, beta):
    return estimation_state_dict(EstUnet(dict(args)), beta, seed)


def map_frame(seed, shape=MAP_SHAPE):
    return np.random.default_rng(seed).uniform(0.0, 1.0, shape).astype(np.float32)


def mean_frame(name, seed):
    """Poisson-Gaussian frames: the SIDD stack is the 256 x 8192 frame cut into 32 blocks (as IterDenoise's lr_cat)."""
    N, H, W = MEAN_CASES[name]
    if name == 'sidd32':
        f, _ = synth_noisy(256, 8192, idx=seed)
        return np.ascontiguousarray(np.stack(np.split(f, 32, axis=-1)))
    f, _ = synth_noisy(H, W, idx=seed)
    return f[None]


def build(args, sd, device):
    net = EstUnet(dict(args))
    net.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return net.to(device)
