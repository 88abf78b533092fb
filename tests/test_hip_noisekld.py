"""GPU: the residual-histogram kernels (csrc/noisehist.hip, include/yond_hip.h M3) and yond_public_amd/noisekld.py against the NumPy
model of tests/noisekld_model.py and the reference's outputs in tests/golden/noisekld.npz.  Counts are integers: every comparison of
counts is `==`.  The KLD of device counts is held to the derived bound of the finish's roundings (noisekld_model.kld_bound).

Shapes: 2 x 2; 4 x 66 (fewer pixels than a wavefront per CFA position, W % 4 != 0: one element per lane); 6 x 10 (a row that ends
inside a 16-byte vector); 36 x 60 = 2160 pixels on the vector path and 34 x 62 = 2108 on the scalar path -- a workgroup takes
YOND_NOISEHIST_BLOCK_ELEMS = 1024 pixels per pass, so both launch three workgroups, the last one partial; B = 3 for the per-frame
offsets of the frames and of the counts.
"""
import os
import re

import numpy as np
import pytest
import torch

import noisekld_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 959.0
SENTINEL = -7777
PAD = 32


def _header_const(name):
    txt = open(os.path.join(ROOT, "include", "yond_hip.h")).read()
    return int(re.search(r"#define\s+" + name + r"\s+(\d+)", txt).group(1))


@pytest.fixture(scope="module")
def NK():
    from yond_public_amd import noisekld
    from yond_public_amd import _lib
    _lib.load()
    return noisekld


@pytest.fixture(scope="module")
def fx(golden):
    return golden("noisekld")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _pair(shape, seed, sigma=0.02):
    """A clean stack with values on the band thresholds, a NaN and negatives, and a noisy one."""
    rs = np.random.RandomState(seed)
    clean = rs.uniform(-0.02, 1.05, shape).astype(np.float32)
    flat = clean.reshape(-1)
    for i, v in enumerate((0.25, 0.5, 0.75, np.nan, np.nextafter(np.float32(0.5), np.float32(0)))):
        flat[(i * 7 + 1) % flat.size] = v
    noisy = (clean + rs.normal(0, sigma, shape) * (1 + 4 * (rs.uniform(size=shape) < 0.02))).astype(np.float32)
    return noisy, clean


def _abi_hist(NK, noisy, clean, thresholds):
    """yond_noise_hist_f32 through the C ABI with the counts inside sentinel margins -> counts, and the margins checked."""
    from yond_public_amd import _lib
    e = NK.kld_edges()
    B = clean.shape[0] if clean.ndim == 3 else 1
    H, W = clean.shape[-2:]
    nb, nbin = len(thresholds) + 1, e.size - 1
    n = B * nb * 4 * nbin
    buf = torch.full((PAD + n + PAD,), SENTINEL, dtype=torch.int64, device='cuda')
    d_n, d_c, d_e = _dev(noisy), _dev(clean), torch.from_numpy(e).cuda()
    d_t = _dev(thresholds) if len(thresholds) else None
    rc = _lib.load().yond_noise_hist_f32(d_n.data_ptr(), d_c.data_ptr(), B, H, W, d_e.data_ptr(), e.size,
                                         d_t.data_ptr() if d_t is not None else None, nb, float(e[1]), 1.0 / (e[2] - e[1]),
                                         buf[PAD:].data_ptr(), None)
    assert rc == 0, rc
    h = _host(buf)
    assert (h[:PAD] == SENTINEL).all() and (h[PAD + n:] == SENTINEL).all()
    return h[PAD:PAD + n].reshape((B, nb, 4, nbin) if clean.ndim == 3 else (nb, 4, nbin))


@pytest.mark.parametrize("shape", [(2, 2), (4, 66), (6, 10), (36, 60), (34, 62), (3, 6, 10), (3, 36, 60), (3, 34, 62)])
def test_counts_equal_the_model(NK, shape):
    assert _header_const("YOND_NOISEHIST_BLOCK_ELEMS") == 1024       # the shapes above are chosen against it
    noisy, clean = _pair(shape, seed=sum(shape))
    t = NK.band_thresholds(4)
    want = M.counts(noisy, clean, thresholds=t)
    got = _abi_hist(NK, noisy, clean, t)
    assert got.shape == want.shape and (got == want).all()
    lib_counts = _host(NK.residual_hist(_dev(noisy), _dev(clean), bands=4))
    assert lib_counts.dtype == np.int64 and (lib_counts == want).all()
    # the marginal run (one band) is the exact sum over the bands; over the CFA positions too it is the model's marginal histogram
    one = _host(NK.residual_hist(_dev(noisy), _dev(clean)))
    assert one.shape == want.shape[:-3] + (1, 4, 66) and (one == want.sum(axis=-3, keepdims=True)).all()
    if len(shape) == 2:
        assert (one.sum((0, 1)) == M.hist_counts(M.residual(noisy, clean))).all()
    else:
        assert not (want[0] == want[1]).all()                        # the frames differ: an offset error shows


@pytest.mark.parametrize("width", [22, 24])
def test_edge_values_frame(NK, fx, width):
    """The golden's edge-value case as a frame (W = 22: one element per lane, W = 24: vectors): residuals on and beside every edge,
    +-1000 and beyond, +-0, NaN, +-inf, under clean values that sit exactly on the band thresholds, beside them, and a NaN.  The
    thresholds are tiny (2^-60 .. 2^-40) so that noisy = clean + r gives r back exactly for all but the residuals of that size."""
    r = fx["edge_values_p"]
    t = np.array([2.0 ** -60, 2.0 ** -50, 2.0 ** -40], np.float32)
    cl_cycle = np.array([0.0, t[0], t[1], t[2], np.nextafter(t[1], np.float32(0)), -0.0, np.nan, np.nextafter(t[2], np.float32(1))], np.float32)
    reps = 8                                                          # every residual meets every clean value
    vals = np.concatenate([np.roll(r, k) for k in range(reps)])
    clean = np.concatenate([np.full(r.size, cl_cycle[k], np.float32) for k in range(reps)])
    pad = (-vals.size) % (2 * width)
    vals, clean = np.concatenate([vals, np.zeros(pad, np.float32)]), np.concatenate([clean, np.zeros(pad, np.float32)])
    clean = clean.reshape(-1, width)
    assert clean.shape[0] % 2 == 0
    with np.errstate(invalid='ignore', over='ignore'):
        noisy = (vals.reshape(-1, width) + clean).astype(np.float32)
    res = M.residual(noisy, clean)
    on_edge = np.isin(res[clean == 0].astype(np.float64), fx["edges"].astype(np.float32).astype(np.float64))
    assert on_edge.sum() >= 60 and np.isnan(clean).any() and (clean == t[1]).any()
    want = M.counts(noisy, clean, thresholds=t)
    got = _host(NK.residual_hist(_dev(noisy), _dev(clean), bands=t))
    assert (got == want).all()
    assert want.sum() < clean.size and (want.sum((1, 2)) > 0).all()      # some pixels are counted nowhere; every band is populated
    # the hint never decides a bin: a useless one gives the same counts
    from yond_public_amd import _lib
    e = NK.kld_edges()
    d_n, d_c, d_e, d_t = _dev(noisy), _dev(clean), torch.from_numpy(e).cuda(), _dev(t)
    for lo, inv in ((0.0, 0.0), (float('nan'), 1.0), (-5.0, 1e9)):
        out = torch.empty(want.shape, dtype=torch.int64, device='cuda')
        assert _lib.load().yond_noise_hist_f32(d_n.data_ptr(), d_c.data_ptr(), 1, clean.shape[0], width, d_e.data_ptr(), e.size,
                                               d_t.data_ptr(), 4, lo, inv, out.data_ptr(), None) == 0
        assert (_host(out) == want).all()


def test_zero_residual_contention(NK):
    """512 x 512 with an identically zero residual: every pixel of a CFA position in ONE bin and one band."""
    clean = np.random.RandomState(0).uniform(0, 1, (512, 512)).astype(np.float32)
    d = _dev(clean)
    got = _host(NK.residual_hist(d, d.clone()))
    e = NK.kld_edges()
    b = int(np.searchsorted(e, 0.0, side='right') - 1)
    assert got.shape == (1, 4, 66) and (got[0, :, b] == clean.size // 4).all() and got.sum() == clean.size
    banded = _host(NK.residual_hist(d, d.clone(), bands=[-1.0, 2.0]))   # every pixel in the middle band of three
    assert banded.shape == (3, 4, 66) and (banded[1, :, b] == clean.size // 4).all() and banded.sum() == clean.size


PG_CONFIGS = {                                   # (K, sigma, exposure, clip): lambda = x * exposure * 959 / K
    'both_regimes': (4.0, 6.0, 1.0, False),      # lambda up to 240: inversion below x = 0.042, PTRS above
    'sigma0': (4.0, 0.0, 1.0, False),
    'clip': (4.0, 6.0, 1.0, True),
    'exposure': (0.5, 2.0, 0.01, False),         # lambda = 19 x: the switch at x = 0.52
    'small_mean': (200.0, 6.0, 1.0, False),      # lambda < 5: inversion only
    'clip_exposure': (0.5, 2.0, 0.01, True),
}


@pytest.fixture(scope="module")
def pg_clean():
    out = {}
    for shape in ((64, 64), (130, 258)):
        rs = np.random.RandomState(shape[1])
        clean = (rs.uniform(0, 1, shape) ** 2).astype(np.float32)          # a third of the pixels below 0.33: both sampler regimes
        flat = clean.reshape(-1)
        flat[5], flat[11], flat[17], flat[23], flat[29] = np.nan, np.inf, -0.01, 0.0, 10.0 / SCALE * 4.0   # (lambda exactly at the switch for K = 4)
        out[shape] = torch.from_numpy(clean).cuda()
    return out


@pytest.mark.parametrize("shape", [(64, 64), (130, 258)])
@pytest.mark.parametrize("cfg", list(PG_CONFIGS))
def test_fused_equals_two_step(NK, pg_clean, shape, cfg):
    from yond_public_amd import pgnoise as PG
    K, sigma, exposure, clip = PG_CONFIGS[cfg]
    clean = pg_clean[shape]
    kw = dict(exposure=exposure, clip=clip)
    got = {}
    for key in (11, 12):
        noisy = PG.add_pg_noise(clean, K, sigma, SCALE, key, [0], **kw)
        two = _host(NK.residual_hist(noisy, clean, bands=3))
        fused = _host(NK.pg_model_hist(clean, K, sigma, SCALE, key, bands=3, **kw))
        assert fused.shape == two.shape == (3, 4, 66) and (fused == two).all()
        # ... and the two-step counts are the model's on the kernel's own noisy frame
        assert (two == M.counts(_host(noisy), _host(clean), thresholds=NK.band_thresholds(3))).all()
        assert two.sum() == clean.numel() - 2                              # the NaN and the inf pixel are counted nowhere
        got[key] = fused
    assert not (got[11] == got[12]).all()                                  # two keys, two realisations


def test_fused_batch_and_slots(NK, pg_clean):
    from yond_public_amd import pgnoise as PG
    clean = torch.stack([pg_clean[(64, 64)], pg_clean[(64, 64)].flip(0), pg_clean[(64, 64)] * 0.5]).contiguous()
    K, sigma = [4.0, 1.0, 8.0], [6.0, 2.0, 0.0]
    noisy = PG.add_pg_noise(clean, K, sigma, SCALE, 99, [5, 6, 7])
    two = _host(NK.residual_hist(noisy, clean, bands=2))
    fused = _host(NK.pg_model_hist(clean, K, sigma, SCALE, 99, bands=2, slots=[5, 6, 7]))
    assert fused.shape == (3, 2, 4, 66) and (fused == two).all()
    assert not (fused == _host(NK.pg_model_hist(clean, K, sigma, SCALE, 99, bands=2))).all()    # the default slots 0, 1, 2 are another stream


@pytest.mark.parametrize("name", M.CASES)
def test_cal_kld_against_golden(NK, fx, name):
    from yond_public_amd.utils import sidd_utils as SU
    assert SU.cal_kld is NK.cal_kld and SU.get_histogram is NK.get_histogram
    p, q = fx[f"{name}_p"], fx[f"{name}_q"]
    dp, dq = _dev(p), _dev(q)
    hp, centers = NK.get_histogram(dp, fx["edges"])
    hq, _ = NK.get_histogram(dq, fx["edges"])
    assert hp.dtype == np.float64 and np.array_equal(hp, fx[f"{name}_hist_p"]) and np.array_equal(hq, fx[f"{name}_hist_q"])
    assert centers.shape == (66,)
    got, ref = NK.cal_kld(dp, dq), float(fx[f"{name}_kld"])
    bound = M.kld_bound(M.hist_counts(p), M.hist_counts(q), p.size, q.size)
    print(f"[noisekld] {name}: device {got:.17g}, reference {ref:.17g}, |delta| {abs(got - ref):.3e}, bound {bound:.3e}")
    assert isinstance(got, float) and abs(got - ref) <= bound


def test_refusals(NK):
    from yond_public_amd import _lib
    lib = _lib.load()
    e = torch.from_numpy(NK.kld_edges()).cuda()
    x = torch.zeros(8, 8, device='cuda')
    out = torch.zeros(4 * 66 * 16, dtype=torch.int64, device='cuda')
    t = torch.zeros(16, device='cuda')
    items = torch.zeros(20, dtype=torch.uint8, device='cuda')
    ok = lambda **k: lib.yond_noise_hist_f32(k.get('noisy', x.data_ptr()), x.data_ptr(), k.get('B', 1), k.get('H', 8), k.get('W', 8),
                                             k.get('edges', e.data_ptr()), k.get('ne', 67), k.get('thr', t.data_ptr()), k.get('nb', 1), 0.0, 0.0,
                                             k.get('counts', out.data_ptr()), None)
    assert ok() == 0
    for bad in (dict(noisy=None), dict(edges=None), dict(counts=None), dict(B=0), dict(H=7), dict(W=6 + 1), dict(H=0), dict(ne=1), dict(nb=0),
                dict(nb=2, thr=None), dict(noisy=x.data_ptr() + 2), dict(edges=e.data_ptr() + 4), dict(H=65536, W=65536)):
        assert ok(**bad) == -1, bad
    assert ok(nb=17) == -2 and ok(ne=258) == -2 and ok(nb=16, ne=200) == -2
    assert lib.yond_pg_noise_hist_f32(x.data_ptr(), 1, 8, 8, None, 0, e.data_ptr(), 67, None, 1, 0.0, 0.0, out.data_ptr(), None) == -1
    assert lib.yond_pg_noise_hist_f32(x.data_ptr(), 1, 8, 8, items.data_ptr(), 2, e.data_ptr(), 67, None, 1, 0.0, 0.0, out.data_ptr(), None) == -1
    torch.cuda.synchronize()
    with pytest.raises(_lib.YondHipError):
        NK.residual_hist(torch.zeros(3, 4, device='cuda'), torch.zeros(3, 4, device='cuda'))
    with pytest.raises(_lib.YondHipError):
        NK.residual_hist(torch.zeros(4, 4), torch.zeros(4, 4))
    with pytest.raises(_lib.YondHipError):
        NK.residual_hist(x, x, bands=20)
