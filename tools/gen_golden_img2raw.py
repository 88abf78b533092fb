"""TEST INFRASTRUCTURE ONLY -- write tests/golden/img2raw.npz by running the reference's sRGB -> raw item.

Run where the reference tree exists (not on the GPU box):

    python tools/gen_golden_img2raw.py

It imports the reference under the stub modules of `oracle/_refimport.py` (used as is) and stores OUTPUTS only, next to the seeded
crops that produced them:
  - eval items of RGB_Img2Raw_Dataset / DIV2K_Img2Raw_Dataset (data_process/yond_datasets.py:277-334, :483-548) for several idx, so
    that all four Bayer patterns appear: hr, lr, wb, ccm, pattern.  Each item's metadata follows setup_seed(idx);
  - explicit-metadata cases through the reference's own unprocess steps (data_process/unprocess.py:80-148) and bayer_aug
    (yond_datasets.py:15-19): a near-white crop (gain mask), the 0.2 / N gain branch, a lock_wb triple, black pixels (1e-8 clamp).
tests/test_img2raw_host.py replays the metadata on CPU, tests/test_hip_img2raw.py the hr planes on the GPU.
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import _refimport  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "img2raw.npz")


def smooth_crop(rng, H, W, dtype, lo=0.0, hi=1.0):
    """A seeded smooth colour crop (sum of a few random sinusoids per channel) scaled to [lo, hi] of the dtype's range."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.zeros((H, W, 3))
    for c in range(3):
        for _ in range(3):
            fy, fx, ph = rng.uniform(0.02, 0.3), rng.uniform(0.02, 0.3), rng.uniform(0, 2 * np.pi)
            img[..., c] += np.sin(fy * y + fx * x + ph)
    img = (img - img.min()) / (img.max() - img.min() + 1e-12)
    img = np.clip(img + rng.normal(0, 0.03, img.shape), 0, 1)
    top = np.iinfo(dtype).max
    return np.round((lo + (hi - lo) * img) * top).astype(dtype)


def main():
    _refimport.import_reference()
    import data_process.yond_datasets as yd
    up = sys.modules["data_process.unprocess"]
    rng = np.random.default_rng(20261016)
    out = {}
    eval_cases, explicit_cases = [], []

    def eval_set(name, cls, crops, idxs, lock_wb=False, subdir=("eval",)):
        with tempfile.TemporaryDirectory() as root:
            d = os.path.join(root, *subdir)
            os.makedirs(d)
            for i, c in enumerate(crops):
                np.save(os.path.join(d, f"crop{i:02d}.npy"), c)
            H, W = crops[0].shape[:2]
            args = dict(root_dir=root, mode="eval", H=H, W=W, command="", lock_wb=lock_wb, gpu_preprocess=False, clip=True,
                        dstname="golden")
            cwd = os.getcwd()
            os.chdir(root)                       # the reference's log() writes under ./
            try:
                ds = getattr(yd, cls)(args)
                ds.sigma = 25 / 255.
                for idx in idxs:
                    it = ds[idx]
                    key = f"{name}_{idx}"
                    eval_cases.append(key)
                    out[key + "_crop"] = crops[idx]
                    out[key + "_hr"] = np.asarray(it["hr"], np.float32)
                    out[key + "_lr"] = np.asarray(it["lr"], np.float32)
                    out[key + "_wb"] = np.asarray(it["wb"], np.float64)
                    out[key + "_ccm"] = np.asarray(it["ccm"], np.float32)
                    out[key + "_pattern"] = np.int64(it["pattern"])
                    out[key + "_idx"] = np.int64(idx)
                    out[key + "_divisor"] = np.float64(255. if cls == "DIV2K_Img2Raw_Dataset" or crops[idx].dtype == np.uint8
                                                      else 65535.)
                    out[key + "_lock_wb"] = np.asarray(lock_wb if lock_wb is not False else [], np.float32).reshape(-1)
            finally:
                os.chdir(cwd)

    eval_set("u8", "RGB_Img2Raw_Dataset", [smooth_crop(rng, 32, 32, np.uint8) for _ in range(6)], range(6))
    eval_set("u16", "RGB_Img2Raw_Dataset", [smooth_crop(rng, 48, 48, np.uint16) for _ in range(4)], range(4))
    eval_set("rect", "RGB_Img2Raw_Dataset", [smooth_crop(rng, 32, 48, np.uint8) for _ in range(3)], (0, 2))
    eval_set("lock", "RGB_Img2Raw_Dataset", [smooth_crop(rng, 32, 32, np.uint8) for _ in range(2)], range(2),
             lock_wb=[[1.0], [2.0], [2.0]])
    # DIV2K divides by 255 whatever the dtype: uint16 levels above 255 saturate
    eval_set("div2k", "DIV2K_Img2Raw_Dataset", [smooth_crop(rng, 32, 32, np.uint16, 0, 400 / 65535) for _ in range(4)], range(4),
             subdir=("npy", "eval"))

    def explicit(name, crop, divisor, rgb2cam, rgb_gain, red, blue, k):
        x = torch.from_numpy(crop.astype(np.float32) / np.float32(divisor))
        t = up.inverse_smoothstep(x)
        t = up.gamma_expansion(t)
        t = up.apply_ccm(t, rgb2cam)
        t = up.safe_invert_gains(t, rgb_gain, red, blue)
        t = torch.clamp(t, min=0.0, max=1.0)
        hr = yd.bayer_aug(up.mosaic(t).numpy(), k=k).transpose(2, 0, 1)
        explicit_cases.append(name)
        out[name + "_crop"] = crop
        out[name + "_hr"] = np.ascontiguousarray(hr, np.float32)
        out[name + "_rgb2cam"] = rgb2cam.numpy()
        out[name + "_gains"] = np.array([rgb_gain.item(), red.item(), blue.item()], np.float32)
        out[name + "_pattern"] = np.int64(k)
        out[name + "_divisor"] = np.float64(divisor)

    def ccm(seed):
        torch.manual_seed(seed)
        return up.random_ccm()

    f = lambda v: torch.tensor([v], dtype=torch.float32)
    white = smooth_crop(rng, 32, 32, np.uint8, 0.9, 1.0)
    white[8:24, 8:24] = 255                      # gray 1 after the CCM: mask 1, the gains are lifted
    explicit("white", white, 255., ccm(1), 1.0 / f(0.8), f(2.0), f(1.8), 1)
    explicit("dim", smooth_crop(rng, 32, 32, np.uint8), 255., ccm(2), 0.2 / f(0.78), f(1.6), f(2.2), 2)
    explicit("lockwb", smooth_crop(rng, 32, 32, np.uint16), 65535., ccm(3), f(1.0), f(2.0), f(2.0), 3)
    black = smooth_crop(rng, 32, 32, np.uint8)
    black[:, :16] = 0
    explicit("black", black, 255., ccm(4), 1.0 / f(0.9), f(2.3), f(1.5), 0)

    out["eval_cases"] = np.array(eval_cases)
    out["explicit_cases"] = np.array(explicit_cases)
    out["sigma"] = np.float64(25 / 255.)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KiB): {len(eval_cases)} eval items, {len(explicit_cases)} explicit cases")


if __name__ == "__main__":
    main()
