"""TEST INFRASTRUCTURE ONLY -- write tests/golden/isp.npz by running the reference's raw -> sRGB functions.

Run where the reference tree exists (not on the GPU box):

    python tools/gen_golden_isp.py

It imports the reference under the stub modules of `oracle/_refimport.py` (used as is), then sets `cv2.cvtColor`,
`cv2.COLOR_BayerBG2RGB_EA` and `cv2.COLOR_BAYER_BG2RGB_EA` on the stub module object to the restated edge-aware demosaic of
tests/isp_model.py (OpenCV is absent: the demosaic is UNPINNED, everything around it is the reference's own code), and calls the
reference's own process_sidd_image (utils/sidd_utils.py:156-180), FastISP (utils/isp_ops.py:171-197) and calculate_ssim
(YOND_SIDD.py:700-721).  Inputs and OUTPUTS only are stored.

The one formula not run from the reference is the sRGB PSNR of the metrics pair: skimage is absent and the stub's
peak_signal_noise_ratio raises, so compare_psnr(dn, hr, data_range=255) is restated as 10 log10(255^2 / mean((dn - hr)^2)) over the
block's three channels.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _refimport  # noqa: E402
import isp_model as M  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "isp.npz")
PATTERNS = {"rggb": [[1, 2], [2, 3]], "grbg": [[2, 1], [3, 2]], "gbrg": [[2, 3], [1, 2]], "bggr": [[3, 2], [2, 1]]}
WB = np.array([[0.5234375, 1.0, 0.6171875]])                       # AsShotNeutral-like: the gains are 1 / wb
# XYZ -> camera matrix whose cam2rgb is [[.86 .11 .03] [.09 .83 .08] [.05 .18 .77]] to three decimals of cst: no entry above 1, so a
# channel reaches the clip at 1 only where all three are saturated -- the band of the scene cases is the white patch alone (0.36 % of
# the 34 x 66 scene; a saturating matrix clips along every edge of the patch and puts 0.9 % at x == 1 exactly).  Its red row sums to
# 1 - 2^-52: a third of the white elements render as 254.  Saturating matrices: the FastISP cases and tests/test_hip_isp.py's shapes.
CST = np.array([[3.968, -2.089, -0.627], [-1.617, 2.557, -0.019], [0.193, -0.727, 1.418]])


def scene(rng, H, W):
    """Smooth sinusoids + sigma 0.04 noise, a 4 x 6 patch of 1.3, one of -0.1 and a flat 4 x 4 patch of 0.5 (all beyond row 6 / column 10)."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = 0.18 + 0.08 * np.sin(0.21 * y + 0.13 * x + 0.4) + 0.04 * np.sin(0.07 * y - 0.31 * x + 1.1) + 0.03 * np.cos(0.5 * x)
    img = img + rng.normal(0, 0.04, img.shape)
    img[8:12, 12:18] = 1.3
    img[16:20, 30:36] = -0.1
    img[24:28, 44:48] = 0.5
    return img.astype(np.float32)


def main():
    ref = _refimport.import_reference()
    cv2 = sys.modules["cv2"]
    assert getattr(cv2, "__stub__", False)
    cv2.cvtColor = M.cv2_cvtcolor
    cv2.COLOR_BayerBG2RGB_EA = cv2.COLOR_BAYER_BG2RGB_EA = 139
    rng = np.random.default_rng(20261017)
    out, sidd_cases, fast_cases = {}, [], []

    def sidd(name, frame, pattern):
        sidd_cases.append(name)
        out[name + "_frame"] = frame
        out[name + "_pattern"] = np.asarray(PATTERNS[pattern], np.int64)
        out[name + "_bgr"] = ref.process_sidd_image(frame.copy(), PATTERNS[pattern], WB, CST)

    base = scene(rng, 34, 66)
    for pat in PATTERNS:
        sidd(f"scene_{pat}", base, pat)
    for (h, w), pat in zip(((2, 2), (2, 34), (6, 10)), ("rggb", "bggr", "grbg")):      # crops in front of the patches: no white
        sidd(f"crop_{h}x{w}", np.ascontiguousarray(base[:h, :w]), pat)
    tie = np.full((12, 12), 0.3, np.float32)
    for yy, xx in ((2, 2), (2, 7), (7, 2), (7, 7)):                                     # a bright pixel at each CFA position
        tie[yy, xx] = 0.9
    sidd("tie", tie, "rggb")

    img4c = rng.uniform(-0.05, 0.7, (16, 24, 4)).astype(np.float32)
    img4c[3:6, 4:9] = 1.1
    fwb = np.array([1.9140625, 1.0, 1.62109375])
    fccm = np.array([[1.71, -0.52, -0.19], [-0.23, 1.58, -0.35], [0.03, -0.61, 1.58]])
    for name, wb, ccm, gamma in (("fast_given", fwb, fccm, 2.2), ("fast_none", None, None, 2.2)):
        fast_cases.append(name)
        out[name + "_rgb"] = np.asarray(ref.FastISP(img4c.copy(), wb, ccm, gamma), np.float64)
    out["fast_img4c"], out["fast_wb"], out["fast_ccm"] = img4c, fwb, fccm

    # the metrics pair: hr and dn = hr + small noise, both rendered; 64 x 64 blocks along the width
    y, x = np.mgrid[0:64, 0:512].astype(np.float64)
    hr = (0.4 + 0.2 * np.sin(0.05 * y + 0.023 * x) + 0.12 * np.cos(0.11 * x - 0.04 * y)).astype(np.float32)
    hr = (np.round(hr * 1023) / 1023).astype(np.float32)                                # (10-bit levels: the fixture compresses)
    dn = (hr + np.round(rng.normal(0, 6, hr.shape)) / 1023).astype(np.float32)
    img_hr = ref.process_sidd_image(hr.copy(), PATTERNS["rggb"], WB, CST)
    img_dn = ref.process_sidd_image(dn.copy(), PATTERNS["rggb"], WB, CST)
    psnr, ssim = [], []
    for b_dn, b_hr in zip(np.split(img_dn, 8, axis=-2), np.split(img_hr, 8, axis=-2)):
        mse = np.mean((b_dn.astype(np.float64) - b_hr.astype(np.float64)) ** 2)
        psnr.append(10 * np.log10(255.0 ** 2 / mse))                                    # compare_psnr(.., data_range=255), restated
        ssim.append(ref.calculate_ssim(b_dn, b_hr))
    out["metrics_hr"], out["metrics_dn"] = hr, dn
    out["metrics_hr_bgr"], out["metrics_dn_bgr"] = img_hr, img_dn
    out["metrics_psnr_rgb"], out["metrics_ssim_rgb"] = np.array(psnr), np.array(ssim)

    out["wb"], out["cst"] = WB, CST
    out["sidd_cases"], out["fast_cases"] = np.array(sidd_cases), np.array(fast_cases)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KiB): {len(sidd_cases)} process_sidd_image cases, {len(fast_cases)} FastISP cases, "
          f"8 metric blocks")


if __name__ == "__main__":
    main()
