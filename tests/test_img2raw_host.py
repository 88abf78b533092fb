"""CPU: the host half of the sRGB -> raw path (yond_public_amd/img2raw.py) against tests/golden/img2raw.npz (the reference's items,
tools/gen_golden_img2raw.py), plus the C ABI's argument checks and the kernel's resource report."""
import ctypes
import os

import numpy as np
import pytest
import torch

from noise_replay import gather_model as _gather_model
from yond_public_amd import img2raw as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g(golden):
    return golden("img2raw")


def _lock(g, key):
    lw = g[key + "_lock_wb"]
    return False if lw.size == 0 else lw.reshape(3, 1).tolist()


def test_eval_metadata_is_the_references(g):
    for key in g["eval_cases"]:
        meta = I.eval_meta(int(g[key + "_idx"]), _lock(g, key))
        assert np.array_equal(I.wb(meta), g[key + "_wb"]), key
        assert np.array_equal(meta["cam2rgb"].numpy(), g[key + "_ccm"]), key


def test_training_draws():
    gen, key = I.train_streams(3, 1)
    assert 0 <= key < 2 ** 32
    n, dim, pats, sig = 4000, 0, [], []
    for _ in range(n):
        meta, p, s = I.sample_item(gen, 5, 50)
        pats.append(p)
        sig.append(s)
        m = meta["rgb2cam"].numpy()
        assert np.all(np.abs(m.sum(axis=1) - 1) < 1e-6)
        assert 1.4 <= meta["red"].item() <= 2.5 and 1.5 <= meta["blue"].item() <= 2.4
        rg = meta["rgb_gain"].item()
        dim += rg < 0.5                       # 0.2 / N(0.8, 0.1) vs 1 / N(0.8, 0.1): disjoint except in far tails
        assert I.gains(meta).shape == (3,) and I.gains(meta)[1].item() == np.float32(1.0 / np.float32(rg))
    assert abs(dim / n - 0.1) < 0.015, dim / n
    assert set(pats) == {0, 1, 2, 3} and max(np.bincount(pats)) < 0.28 * n
    sig = np.array(sig) * 255
    assert sig.min() >= 5 and sig.max() <= 50
    assert abs(np.log(sig).mean() - (np.log(5) + np.log(50)) / 2) < 0.03       # log-uniform
    # no_bayeraug: pattern 0; lock_wb: the triple, only the CCM drawn
    meta, p, _ = I.sample_item(gen, 5, 50, lock_wb=[1.0, 2.0, 2.5], bayer_aug=False)
    assert p == 0 and (meta["rgb_gain"].item(), meta["red"].item(), meta["blue"].item()) == (1.0, 2.0, 2.5)
    # a (epoch, rank) pair is its own stream, reproducible
    a, b, c = I.train_streams(3, 1)[0], I.train_streams(3, 1)[0], I.train_streams(3, 0)[0]
    ra, rb, rc = (I.sample_meta(x)["rgb2cam"] for x in (a, b, c))
    assert torch.equal(ra, rb) and not torch.equal(ra, rc)


def _ref_curve(x):
    """unprocess.py:80-95 per pixel, restated in torch float32."""
    x = torch.clamp(x, min=0.0, max=1.0)
    x = 0.5 - torch.sin(torch.asin(1.0 - 2.0 * x) / 3.0)
    return torch.clamp(x, min=1e-8) ** 2.2


def test_transfer_tables(g):
    for key in list(g["eval_cases"]) + list(g["explicit_cases"]):
        crop, div = g[key + "_crop"], float(g[key + "_divisor"])
        t = I.curve_host(crop.dtype, div)
        assert t.shape == ((256,) if crop.dtype == np.uint8 else (65536,)) and t.dtype == torch.float32
        per_pixel = _ref_curve(torch.from_numpy(crop.astype(np.float32) / np.float32(div)))
        assert torch.equal(t[torch.from_numpy(crop.astype(np.int64))], per_pixel), key
    lv = torch.arange(256, dtype=torch.float32) / 255.
    assert torch.equal(I.curve_host(np.uint8, 255.), _ref_curve(lv))
    assert I.curve_host(np.uint8, 255.)[0].item() == np.float32(1e-8) ** np.float32(2.2)


def test_gather_model_matches_the_reference(g):
    """The index map and arithmetic the kernel implements, checked on CPU against the reference's items (the GPU test checks the
    kernel itself)."""
    worst = 0.0
    for key in g["eval_cases"]:
        crop = g[key + "_crop"]
        meta = I.eval_meta(int(g[key + "_idx"]), _lock(g, key))
        table = I.curve_host(crop.dtype, float(g[key + "_divisor"])).numpy()
        hr = _gather_model(crop, table, meta["rgb2cam"].numpy(), I.gains(meta).numpy(), int(g[key + "_pattern"]))
        assert hr.shape == g[key + "_hr"].shape, key
        worst = max(worst, float(np.abs(hr - g[key + "_hr"]).max()))
    for key in g["explicit_cases"]:
        crop = g[key + "_crop"]
        rg, red, blue = (torch.tensor([v]) for v in g[key + "_gains"])
        gain = I.gains({"rgb_gain": rg, "red": red, "blue": blue}).numpy()
        table = I.curve_host(crop.dtype, float(g[key + "_divisor"])).numpy()
        hr = _gather_model(crop, table, g[key + "_rgb2cam"], gain, int(g[key + "_pattern"]))
        worst = max(worst, float(np.abs(hr - g[key + "_hr"]).max()))
    assert worst <= 2e-6, worst


def test_fixture_covers_the_cases(g):
    pats = {int(g[k + "_pattern"]) for k in g["eval_cases"]}
    assert pats == {0, 1, 2, 3}
    assert {g[k + "_crop"].dtype for k in g["eval_cases"]} == {np.dtype(np.uint8), np.dtype(np.uint16)}
    assert any(g[k + "_crop"].shape[0] != g[k + "_crop"].shape[1] for k in g["eval_cases"])
    white = g["white_hr"]
    assert white.max() == 1.0 and g["white_gains"][0] > 1   # the mask lifts white pixels the gains (all < 1) would dim
    assert g["dim_gains"][0] < 0.5                # the 0.2 / N branch
    assert (g["black_crop"] == 0).any()


def test_crop_kind(tmp_path):
    s, p, m = (tmp_path / n for n in ("s", "p", "m"))
    for d in (s, p, m):
        d.mkdir()
    np.save(s / "a.npy", np.zeros((8, 8, 3), np.uint8))
    np.save(s / "b.npy", np.zeros((8, 8, 3), np.uint16))
    np.save(p / "a.npy", np.zeros((4, 4, 4), np.float32))
    np.save(p / "b.npy", np.zeros((4, 4, 4), np.float32))
    np.save(p / "c.npy", np.zeros((8, 8, 3), np.float32))      # float (H, W, 3) is not an sRGB crop
    np.save(m / "a.npy", np.zeros((8, 8, 3), np.uint8))
    np.save(m / "b.npy", np.zeros((4, 4, 4), np.float32))
    ls = lambda d: sorted(str(x) for x in d.glob("*.npy"))
    assert I.crop_kind(ls(s)) == "srgb"
    assert I.crop_kind(ls(p)) == "packed"
    assert I.crop_kind([]) is None
    with pytest.raises(ValueError, match="sRGB crops.*packed raw"):
        I.crop_kind(ls(m))


def test_patch_layout():
    p = I.plan([0, 1234567890123], [I.eval_meta(0), I.eval_meta(1)], [1, 3], [0.1, 0.2], 77, [5, 6])
    assert p.dtype.itemsize == 72 and p.dtype.fields["offset"][1] == 64 and p.dtype.fields["sigma"][1] == 48
    assert list(p["pattern"]) == [1, 3] and list(p["slot"]) == [5, 6] and p["key"][1] == 77 and p["offset"][1] == 1234567890123


def test_abi_argument_checks_without_gpu():
    import __graft_entry__ as ge
    ge.build()
    from yond_public_amd import _lib
    lib = _lib.load()
    f = lib.yond_img2raw_f32
    d = ctypes.c_void_p(16)                       # never dereferenced: every call below is refused before a launch
    ok = dict(crops=d, n=3 * 64, dtype=0, H=8, W=8, curve=d, patches=d, B=1, pattern=0, clip=1, hr=d, lr=d, sigma=None, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(*a.values())
    for name in ("crops", "curve", "patches", "hr", "lr"):
        assert call(**{name: None}) == -1, name
    assert call(H=7) == -1 and call(W=9) == -1 and call(H=0) == -1
    assert call(B=0) == -1
    assert call(dtype=2) == -1 and call(dtype=-1) == -1
    assert call(pattern=4) == -1 and call(pattern=-2) == -1
    assert call(pattern=-1, H=8, W=16) == -1


def test_kernel_has_no_spills():
    from yond_public_amd import build as B
    B.build_lib(verbose=False)
    rep = [r for r in B.resource_report() if "img2raw" in r["name"]]
    if not B.resource_report():
        pytest.skip("a shipped library without its object directory or link-time report: nothing to check here")
    assert len(rep) == 2, rep                     # the uint8 and uint16 instantiations
    assert not [r for r in rep if r.get("vgpr_spill", 0) or r.get("sgpr_spill", 0) or r.get("scratch", 0)], rep
