"""CPU: the float model of the raw-crop kernel (tests/rawcrop_model.py) and the planner's draws (yond_public_amd/rawcrop.py) against
the reference's SID_Raw_Dataset items recorded in tests/golden/rawcrop.npz; the planner's and the dataset's refusals."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import rawcrop_model as M
from yond_public_amd import rawcrop as R


class LegacyDraws:
    """The reference's generators after np.random.seed(s) / torch.manual_seed(s), as rawcrop.sample_item takes them."""

    def __init__(self, seed):
        self.rs, self.gen = np.random.RandomState(seed), torch.Generator().manual_seed(seed)

    def integers(self, n, size=None):
        return self.rs.randint(n, size=size)

    def random(self):
        return self.rs.rand()


def test_model_equals_the_reference_hr_bit_for_bit(golden):
    g = golden("rawcrop")
    bl, wp = g["bl_wp"]
    n = 0
    for kind in ("train", "eval"):
        for c in M.golden_cases(g, kind):
            rgb, g0, g2 = M.case_gains(c)
            ps = c["patch_size"] if kind == "train" else None
            if kind == "train":
                got = M.patches_hr(c["bayer"], bl, wp, c["pattern"], c["vst_aug"], c["y0"], c["x0"], ps, rgb, g0, g2, c["clip"])
            else:                                  # the whole frame: rectangular, so straight from the model's steps
                got = M.frame_hr(c["bayer"], bl, wp, c["pattern"], c["vst_aug"])[None] * np.float32(rgb)
                got[:, 0] = (got[:, 0].astype(np.float64) * g0).astype(np.float32)
                got[:, 2] = (got[:, 2].astype(np.float64) * g2).astype(np.float32)
                got = got.clip(0, 1) if c["clip"] else got
            assert got.shape == c["hr"].shape and got.dtype == np.float32, c["name"]
            assert np.array_equal(got.view(np.uint32), c["hr"].view(np.uint32)), (c["name"], np.abs(got - c["hr"]).max())
            n += 1
    assert n == 80
    seen = {(c["pattern"], c["vst_aug"], c["gains_drawn"]) for c in M.golden_cases(g, "train")}
    assert {s[0] for s in seen} == {0, 1, 2, 3} and {s[1] for s in seen} == {0, 1} and {s[2] for s in seen} == {0, 1}


def test_eval_draws_equal_the_reference_wb_bit_for_bit(golden):
    g = golden("rawcrop")
    coins = set()
    for c in M.golden_cases(g, "eval"):
        d = R.eval_draws(c["frame"], c["wb_in"], lock_wb=bool(c["lock_wb"]))
        assert d["pattern"] == c["pattern"] == c["frame"] % 4 and d["vst_aug"] == (c["frame"] // 4) % 2
        assert np.array_equal(d["wb"].view(np.uint64), c["wb"].view(np.uint64)), c["name"]
        assert (d["gains"] is not None) == bool(c["gains_drawn"])
        if c["gains_drawn"]:
            assert np.array_equal(d["gains"], c["gains"])
            rgb, g0, g2 = M.case_gains(c)
            assert (d["rgb_gain"], d["gain0"], d["gain2"]) == (rgb, g0, g2)
        if not c["lock_wb"]:
            coins.add(c["gains_drawn"])
    assert coins == {0, 1}


def test_train_draws_replay_through_the_planner(golden):
    g = golden("rawcrop")
    lo, hi = g["sigma_range"]
    for c in M.golden_cases(g, "train"):
        H, W = c["bayer"].shape
        d = R.sample_item(LegacyDraws(c["seed"]), H // 2, W // 2, c["patch_size"], c["crop_per_image"],
                          "non-overlapped" if c["non_overlapped"] else "random", lo, hi, lock_wb=bool(c["lock_wb"]), wb=c["wb_in"])
        assert (d["pattern"], d["vst_aug"], d["y0"], d["x0"]) == (c["pattern"], c["vst_aug"], c["y0"], c["x0"]), c["name"]
        assert d["sigma"] == c["sigma"]
        assert (d["gains"] is not None) == bool(c["gains_drawn"])
        assert np.array_equal(d["wb"].view(np.uint64), c["wb"].view(np.uint64))
        if c["gains_drawn"]:
            assert np.array_equal(d["gains"], c["gains"])
        p = R.plan([0], [d], H, W, c["patch_size"], 7, np.arange(c["crop_per_image"]))
        assert p["y0"].tolist() == c["y0"] and p["x0"].tolist() == c["x0"] and set(p["pattern"]) == {c["pattern"]}
        rgb, g0, g2 = M.case_gains(c)
        assert p["rgb_gain"][0] == rgb and p["gain0"][0] == g0 and p["gain2"][0] == g2
        assert p["slot"].tolist() == list(range(c["crop_per_image"])) and set(p["key"]) == {7}


def test_torch_generator_draws_stay_inside_the_frame():
    gen = torch.Generator().manual_seed(3)
    for croptype in ("random", "non-overlapped"):
        seen = set()
        for _ in range(200):                       # 16 combinations: one missing after 200 draws has probability < 1e-4
            d = R.sample_item(gen, 6, 10, 3, 3, croptype, 5, 50)
            ho, wo = (10, 6) if d["pattern"] & 1 else (6, 10)
            assert all(0 <= y <= ho - 3 for y in d["y0"]) and all(0 <= x <= wo - 3 for x in d["x0"])
            assert 5 / 255. <= d["sigma"] <= 50 / 255.
            R.plan([0], [d], 12, 20, 3, 1, 0)
            seen.add((d["pattern"], d["vst_aug"], d["gains"] is None))
        assert len(seen) == 16
    d = R.sample_item(gen, 6, 10, 3, 3, "random", 5, 50, lock_wb=True)
    assert d["gains"] is None and d["rgb_gain"] == 1 and d["gain0"] == 1 and d["gain2"] == 1


def test_patch_struct_layout():
    f = R.PATCH_DTYPE.fields
    assert R.PATCH_DTYPE.itemsize == 64
    assert [f[k][1] for k in ("frame", "y0", "x0", "pattern", "vst_aug", "rgb_gain", "gain0", "gain2", "sigma", "key", "slot")] == \
        [0, 8, 12, 16, 20, 24, 32, 40, 48, 52, 56]


# -- refusals, no GPU ---------------------------------------------------------------------------------------------------------
def _frames(d, shapes, dtype=np.uint16):
    os.makedirs(d, exist_ok=True)
    paths = []
    for i, s in enumerate(shapes):
        paths.append(os.path.join(d, f"f{i}.npy"))
        np.save(paths[-1], np.full(s, 200, dtype))
    return paths


def test_frames_of_mixed_shape_or_odd_size_raise(tmp_path):
    with pytest.raises(ValueError, match=r"share shape and dtype.*f0\.npy.*f1\.npy"):
        R.frame_shape(_frames(str(tmp_path / "a"), [(12, 20), (20, 12)]))
    with pytest.raises(ValueError, match=r"share shape and dtype"):
        R.frame_shape(_frames(str(tmp_path / "b"), [(12, 20)]) + _frames(str(tmp_path / "c"), [(12, 20)], np.float32))
    with pytest.raises(ValueError, match=r"H and W must be even, got 11 x 20 \(f0\.npy"):
        R.frame_shape(_frames(str(tmp_path / "d"), [(11, 20)]))
    with pytest.raises(ValueError, match="uint16 or float32"):
        R.frame_shape(_frames(str(tmp_path / "e"), [(12, 20)], np.uint8))
    assert R.frame_shape(_frames(str(tmp_path / "f"), [(12, 20)] * 2, np.float32)) == (12, 20, np.dtype(np.float32))


def test_plan_refuses_a_crop_outside_the_rotated_frame():
    ok = dict(pattern=1, vst_aug=0, y0=[6], x0=[2], rgb_gain=1, gain0=1., gain2=1., sigma=.1)     # 12 x 20 rotated: packed 10 x 6
    assert len(R.plan([0], [ok], 12, 20, 4, 1, 0)) == 1
    for bad in (dict(ok, pattern=0), dict(ok, x0=[3]), dict(ok, y0=[7]), dict(ok, y0=[-1]), dict(ok, x0=[-1]), dict(ok, pattern=4)):
        with pytest.raises(ValueError):
            R.plan([0], [bad], 12, 20, 4, 1, 0)


def _sid_args(root, **kw):
    return dict(dict(root_dir=str(root), mode="train", H=12, W=20, patch_size=4, crop_per_image=2, croptype="non-overlapped",
                     sigma_min=5, sigma_max=50, clip=True), **kw)


def test_dataset_refuses_too_many_non_overlapped_crops(tmp_path, monkeypatch):
    from yond_public_amd import trainer_AWGN as TA
    monkeypatch.chdir(tmp_path)
    _frames(str(tmp_path / "d" / "train"), [(12, 20)] * 2)
    assert len(TA.SID_Raw_Dataset(_sid_args(tmp_path / "d"))) == 2
    with pytest.raises(ValueError, match="non-overlapped.*only 2 cells"):
        TA.SID_Raw_Dataset(_sid_args(tmp_path / "d", crop_per_image=3))
    assert len(TA.SID_Raw_Dataset(_sid_args(tmp_path / "d", crop_per_image=3, croptype="random"))) == 2
    with pytest.raises(ValueError, match="share shape"):
        _frames(str(tmp_path / "m" / "train"), [(12, 20), (20, 12)])
        TA.SID_Raw_Dataset(_sid_args(tmp_path / "m"))
    with pytest.raises(NotImplementedError, match="on the GPU"):
        TA.SID_Raw_Dataset(_sid_args(tmp_path / "d"))[0]


def test_dataset_frame_list_info_file_glob_and_sidecar(tmp_path, monkeypatch):
    from yond_public_amd import trainer_AWGN as TA
    monkeypatch.chdir(tmp_path)
    paths = _frames(str(tmp_path / "d" / "train"), [(12, 20)] * 3)
    with open(paths[1][:-4] + ".json", "w") as f:
        json.dump({"wb": [2.0, 1, 1.5], "ccm": np.eye(3).tolist()}, f)
    ds = TA.SID_Raw_Dataset(_sid_args(tmp_path / "d"))                                    # no infos/: the glob, sorted
    assert ds.datapath == sorted(paths) and ds.names == ["f0", "f1", "f2"]
    assert [list(w) for w in ds.wbs] == [[1, 1, 1], [2, 1, 1.5], [1, 1, 1]] and np.array_equal(ds.ccms[1], np.eye(3))
    assert ds.ccms[0] is None
    os.makedirs(tmp_path / "infos")
    infos = [dict(long=paths[2], name="two", wb=np.array([1.9, 1, 1.7]), ccm=np.eye(3)), dict(long=paths[0], name="zero", wb=[2.1, 1, 1.6], ccm=np.eye(3))]
    with open(tmp_path / "infos" / "SID_train.info", "wb") as f:
        pickle.dump(infos, f)
    ds = TA.SID_Raw_Dataset(_sid_args(tmp_path / "d"))                                    # the reference's info file wins
    assert ds.datapath == [paths[2], paths[0]] and ds.names == ["two", "zero"] and list(ds.wbs[1]) == [2.1, 1, 1.6]
    os.rename(tmp_path / "infos" / "SID_train.info", tmp_path / "elsewhere.info")
    ds = TA.SID_Raw_Dataset(_sid_args(tmp_path / "d", info_file=str(tmp_path / "elsewhere.info")))
    assert ds.names == ["two", "zero"]
    with pytest.raises(FileNotFoundError, match="--synthetic"):
        TA.SID_Raw_Dataset(_sid_args(tmp_path / "nothing"))
    syn = TA.SID_Raw_Dataset(_sid_args(tmp_path / "nothing", wp=16383, bl=512), synthetic=3)
    assert len(syn) == 3 and syn.frames[0].shape == (12, 20) and syn.frames[0].dtype == np.uint16
    assert 512 <= syn.frames[0].min() and syn.frames[2].max() <= 16383 and not np.array_equal(syn.frames[0], syn.frames[1])
