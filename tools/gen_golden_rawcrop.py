"""TEST INFRASTRUCTURE ONLY -- write tests/golden/rawcrop.npz by running the reference's SID_Raw_Dataset.__getitem__.

Run where the reference tree exists (not on the GPU box):

    python tools/gen_golden_rawcrop.py

It imports the reference under the stub modules of `oracle/_refimport.py` (used as is), builds the dataset in a temporary directory
that holds tiny seeded uint16 Bayer frames and an `infos/SID_<mode>.info` written here, and stores OUTPUTS only, next to the frames
that produced them (12 x 20 and 20 x 12, bl 512, wp 16383, DN below bl, above wp, exactly bl and exactly wp among them):
  - train items (data_process/yond_datasets.py:153-212) after np.random.seed(s) / torch.manual_seed(s): hr, pattern, vst_aug, the
    post-swap crop origins, sigma, the item's wb and what random_gains() returned (the function is wrapped where the dataset
    module looks it up), for both croptypes, lock_wb on and off, clip on and off.  patch_size 4 with crop_per_image 3 for random
    crops; the 'non-overlapped' grid of a 6 x 10 packed frame has two cells of 4, where the reference can cut no third patch, so
    that croptype runs with (patch_size 4, crop_per_image 2) and (patch_size 3, crop_per_image 3);
  - eval items for idx 0..7, so that all four patterns and both outcomes of the gain coin appear: hr (the whole frame), wb, and
    the vst_aug the reference happened to draw before it seeded.
Every call gets a fresh wb array: the reference writes the jittered gains back into its info entry (:190-191).
tests/test_rawcrop_model.py replays all of it on the CPU, tests/test_hip_rawcrop.py the hr planes on the GPU.
The archive's members carry a fixed date, so a second run writes the same bytes.
"""
import io
import os
import pickle
import sys
import tempfile
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import _refimport  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "rawcrop.npz")
BL, WP = 512, 16383
META_FIELDS = ("pattern", "vst_aug", "shape", "frame", "patch_size", "crop_per_image", "lock_wb", "clip", "non_overlapped", "seed",
               "gains_drawn")
SHAPES = [(12, 20), (20, 12)]
N_PER_SHAPE = 8


def frames_of(rng, shape, n):
    out = []
    for _ in range(n):
        f = rng.integers(300, 16600, shape).astype(np.uint16)           # below bl .. above wp
        f.reshape(-1)[rng.choice(f.size, 8, replace=False)] = [BL, WP, 0, 65535, BL - 1, BL + 1, WP - 1, WP + 1]
        out.append(f)
    return out


def write_npz(path, arrays):
    """np.savez_compressed with a fixed member date (the archive is then a function of its contents alone)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    _refimport.import_reference()
    import data_process.yond_datasets as yd
    rng = np.random.default_rng(20261020)
    out, train_cases, eval_cases = {}, [], []
    seen = []                                                            # random_gains() return values, in call order
    inner = yd.random_gains

    def recording_gains():
        g = inner()
        seen.append(np.array([t.item() for t in g], np.float32))
        return g
    yd.random_gains = recording_gains

    cwd = os.getcwd()
    try:
        for si, shape in enumerate(SHAPES):
            frames = frames_of(rng, shape, N_PER_SHAPE)
            wbs = [np.array([rng.uniform(1.6, 2.4), 1.0, rng.uniform(1.4, 2.0)]) for _ in frames]
            for i, f in enumerate(frames):
                out[f"frame_s{si}_{i}"] = f
                out[f"wb_s{si}_{i}"] = wbs[i]
            with tempfile.TemporaryDirectory() as root:
                os.makedirs(os.path.join(root, "infos"))
                paths = []
                for i, f in enumerate(frames):
                    paths.append(os.path.join(root, f"frame{i:02d}.npy"))
                    np.save(paths[-1], f)
                infos = [dict(long=p, name=f"frame{i:02d}", wb=wbs[i].copy(), ccm=np.eye(3, dtype=np.float32)) for i, p in enumerate(paths)]
                for mode in ("train", "eval"):
                    with open(os.path.join(root, "infos", f"SID_{mode}.info"), "wb") as fh:
                        pickle.dump(infos, fh)
                os.chdir(root)                       # the reference opens infos/ relative to the working directory

                def dataset(mode, **kw):
                    args = dict(root_dir=root, mode=mode, H=shape[0], W=shape[1], wp=WP, bl=BL, command="", gpu_preprocess=False,
                                sigma_min=5, sigma_max=50, croptype="random", patch_size=4, crop_per_image=3, lock_wb=False, clip=False)
                    args.update(kw)
                    return yd.SID_Raw_Dataset(args), args

                def record(rows, it, args, idx, ds, seed=-1, train=False):
                    rows.append(dict(
                        hr=np.asarray(it["hr"], np.float32),
                        meta=[int(it["pattern"]), int(bool(it["vst_aug"])), si, idx, args["patch_size"], args["crop_per_image"],
                              int(args["lock_wb"] is not False), int(bool(args["clip"])), int(args["croptype"] == "non-overlapped"), seed,
                              int(bool(seen))],
                        wb=[float(np.asarray(v).reshape(-1)[0]) for v in it["wb"]],
                        gains=seen[-1] if seen else np.zeros(3, np.float32),
                        y0=list(ds.h_start) if train else [0], x0=list(ds.w_start) if train else [0],
                        sigma=float(it["sigma"])))

                # -- train items
                configs = [dict(croptype="random", patch_size=4, crop_per_image=3),
                           dict(croptype="non-overlapped", patch_size=4, crop_per_image=2),
                           dict(croptype="non-overlapped", patch_size=3, crop_per_image=3)]
                for ci, cfg in enumerate(configs):
                    for lock_wb in (False, True):
                        for clip in (False, True):
                            ds, args = dataset("train", lock_wb=lock_wb, clip=clip, **cfg)
                            for n in range(2):
                                idx = int(rng.integers(len(frames)))
                                seed = int(rng.integers(1 << 30))
                                ds.infos[idx]["wb"] = wbs[idx].copy()
                                del seen[:]
                                np.random.seed(seed)
                                torch.manual_seed(seed)
                                it = ds[idx]
                                record(train_cases, it, args, idx, ds, seed, train=True)
                # -- eval items
                for lock_wb, clip in ((False, False), (True, True)):
                    ds, args = dataset("eval", lock_wb=lock_wb, clip=clip)
                    ds.sigma = 25 / 255.
                    for idx in range(N_PER_SHAPE):
                        ds.infos[idx]["wb"] = wbs[idx].copy()
                        del seen[:]
                        it = ds[idx]
                        record(eval_cases, it, args, idx, ds)
                os.chdir(cwd)
    finally:
        os.chdir(cwd)
        yd.random_gains = inner

    for kind, rows in (("train", train_cases), ("eval", eval_cases)):
        # one member per field, the cases along the first axis (META_FIELDS names the columns of *_meta); the hr planes, whose
        # shapes differ, lie flattened end to end with case i at [hr_off[i], hr_off[i + 1]) as (crops, 4, ps or h', ps or w')
        ncrop = max(len(r["y0"]) for r in rows)
        out[kind + "_meta"] = np.array([r["meta"] for r in rows], np.int64)
        out[kind + "_wb"] = np.array([r["wb"] for r in rows], np.float64)
        out[kind + "_gains"] = np.array([r["gains"] for r in rows], np.float32)
        out[kind + "_sigma"] = np.array([r["sigma"] for r in rows], np.float64)
        out[kind + "_y0"] = np.array([r["y0"] + [-1] * (ncrop - len(r["y0"])) for r in rows], np.int64)
        out[kind + "_x0"] = np.array([r["x0"] + [-1] * (ncrop - len(r["x0"])) for r in rows], np.int64)
        out[kind + "_hr"] = np.concatenate([r["hr"].reshape(-1) for r in rows])
        out[kind + "_hr_off"] = np.cumsum([0] + [r["hr"].size for r in rows]).astype(np.int64)
        out[kind + "_hr_shape"] = np.array([r["hr"].shape for r in rows], np.int64)
    out["bl_wp"] = np.array([BL, WP], np.float64)
    out["sigma_range"] = np.array([5, 50], np.float64)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    write_npz(OUT, out)
    pats = sorted({r["meta"][0] for r in train_cases})
    coin = sorted({bool(r["meta"][10]) for r in eval_cases if not r["meta"][6]})
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KiB): {len(train_cases)} train items (patterns {pats}), "
          f"{len(eval_cases)} eval items (gain coin outcomes {coin})")


if __name__ == "__main__":
    main()
