"""NumPy model of yond_rawcrop_f32's signal path (include/yond_hip.h, I4; steps 1-6 and 8 of the kernel: everything but the noise),
with exactly the dtypes of the reference's SID_Raw_Dataset.__getitem__ (data_process/yond_datasets.py:162-210).  It takes the
planner's draws explicitly and is written with whole-array NumPy calls, not per element: the kernel's index maps are checked against
np.rot90 and the reshape of bayer2rggb, not against themselves."""
import numpy as np


def pack(bayer):
    """bayer2rggb (utils/isp_ops.py:57-59) as (4, h, w): channel 2 * dy + dx."""
    H, W = bayer.shape
    return bayer.reshape(H // 2, 2, W // 2, 2).transpose(1, 3, 0, 2).reshape(4, H // 2, W // 2)


def frame_hr(frame, bl, wp, pattern, vst_aug):
    """Steps 1-4 for a whole frame: (4, h', w') float32 of the rotated frame."""
    den = np.float32(np.float32(wp) - np.float32(bl))
    v = (frame.astype(np.float32) - np.float32(bl)) / den
    v = pack(np.rot90(v, k=pattern, axes=(-2, -1)))
    v = np.minimum(np.maximum(v, np.float32(0)), np.float32(1))
    return np.sqrt(v) if vst_aug else v


def patches_hr(frame, bl, wp, pattern, vst_aug, y0, x0, ps, rgb_gain=1.0, gain0=1.0, gain2=1.0, clip=False):
    """hr of the patches cut at packed origins (y0[i], x0[i]) of the rotated frame: (n, 4, ps, ps) float32.  Steps 5-6: times
    rgb_gain in float32, channels 0 and 2 times a float64 gain rounded once to float32; step 8: the [0, 1] clamp."""
    whole = frame_hr(frame, bl, wp, pattern, vst_aug)
    out = np.stack([whole[:, y:y + ps, x:x + ps] for y, x in zip(y0, x0)]).astype(np.float32)
    assert out.shape == (len(y0), 4, ps, ps), "a crop leaves the frame"
    out = out * np.float32(rgb_gain)
    out[:, 0] = (out[:, 0].astype(np.float64) * np.float64(gain0)).astype(np.float32)
    out[:, 2] = (out[:, 2].astype(np.float64) * np.float64(gain2)).astype(np.float32)
    if clip:
        out = np.minimum(np.maximum(out, np.float32(0)), np.float32(1))
    return out


META_FIELDS = ("pattern", "vst_aug", "shape", "frame", "patch_size", "crop_per_image", "lock_wb", "clip", "non_overlapped", "seed",
               "gains_drawn")                     # the columns of *_meta in tests/golden/rawcrop.npz (tools/gen_golden_rawcrop.py)


def golden_cases(g, kind):
    """The recorded reference items of tests/golden/rawcrop.npz, kind 'train' or 'eval', as dicts: the META_FIELDS, `bayer` (the
    frame), `wb_in` (the frame's white balance), and the reference's `hr`, `wb`, `gains` (rgb, red, blue; meaningful when
    gains_drawn), `sigma`, `y0` / `x0` (post-swap origins; [0] for an eval item, which is the whole frame)."""
    meta, off = g[kind + "_meta"], g[kind + "_hr_off"]
    for i in range(len(meta)):
        c = dict(zip(META_FIELDS, (int(v) for v in meta[i])))
        n = c["crop_per_image"] if kind == "train" else 1
        c.update(name=f"{kind}{i}", bayer=g[f"frame_s{c['shape']}_{c['frame']}"], wb_in=g[f"wb_s{c['shape']}_{c['frame']}"],
                 hr=g[kind + "_hr"][off[i]:off[i + 1]].reshape(g[kind + "_hr_shape"][i]), wb=g[kind + "_wb"][i],
                 gains=g[kind + "_gains"][i], sigma=float(g[kind + "_sigma"][i]),
                 y0=[int(v) for v in g[kind + "_y0"][i][:n]], x0=[int(v) for v in g[kind + "_x0"][i][:n]])
        yield c


def case_gains(c):
    """(rgb_gain float32, gain0, gain2 float64) of a recorded item: yond_datasets.py:184-186 on the recorded random_gains()."""
    if not c["gains_drawn"]:
        return np.float32(1), 1.0, 1.0
    rgb, red, blue = (np.float32(v) for v in c["gains"])
    return rgb, float(np.float64(c["wb_in"][0]) / red), float(np.float64(c["wb_in"][2]) / blue)
