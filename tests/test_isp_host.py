"""CPU: the host side of the sRGB renderer (yond_public_amd/isp.py), the sRGB meters of distributed.MetricSums and the
driver's --fig flag."""
import numpy as np
import pytest

import isp_model as M


def test_threshold_table():
    from yond_public_amd import isp
    t = isp.threshold_table()
    assert t.shape == (255,) and t.dtype == np.float64
    assert (np.diff(t) > 0).all() and t[0] > 0 and t[-1] <= 1.0
    np.testing.assert_array_equal(t, M.thresholds())


def test_cam2rgb_rows_sum_to_one(golden):
    from yond_public_amd import isp
    for cst in (golden("isp")["cst"], np.array([[0.9142, -0.3268, -0.0871], [-0.4537, 1.3009, 0.1652], [-0.0913, 0.2446, 0.6104]])):
        m = isp.cam2rgb(cst)
        np.testing.assert_allclose(m.sum(axis=-1), 1.0, rtol=0, atol=4e-16)
        np.testing.assert_array_equal(m, M.cam2rgb(cst))
    np.testing.assert_allclose(isp.cam2rgb(np.linalg.inv(isp.RGB2XYZ)), np.eye(3), atol=1e-12)


def test_flip_flags_per_pattern():
    from yond_public_amd import isp
    assert isp.flip_flags([[1, 2], [2, 3]]) == (False, False)
    assert isp.flip_flags([[2, 1], [3, 2]]) == (True, False)
    assert isp.flip_flags([[2, 3], [1, 2]]) == (False, True)
    assert isp.flip_flags(np.array([[3, 2], [2, 1]])) == (True, True)
    for bad in ([[1, 2], [3, 2]], [[0, 1], [1, 2]], 'rggb', [1, 2, 3]):
        with pytest.raises(ValueError):
            isp.flip_flags(bad)
    # the flips bring every pattern to RGGB
    for pat, (lr, ud) in M.FLIPS.items():
        a = np.array(pat)
        a = a[:, ::-1] if lr else a
        a = a[::-1, :] if ud else a
        assert a.tolist() == [[1, 2], [2, 3]]


def test_fast_gain_follows_numpy_promotion():
    from yond_public_amd import isp
    assert isp._fast_gain(1.9) == float(np.float32(1.9)) and isp._fast_gain(2) == 2.0
    assert isp._fast_gain(np.float64(1.9)) == 1.9 and isp._fast_gain(np.float32(1.9)) == float(np.float32(1.9))
    x = np.float32(0.3712345)
    assert (np.array([x]) * 1.9).dtype == np.float32 and (np.array([x]) * np.float64(1.9)).dtype == np.float64


def test_metric_sums_default_is_todays_vector():
    from yond_public_amd import distributed as D
    s = D.MetricSums(2)
    assert s.vec.shape == (7,) and s.vec.dtype.is_floating_point and s.vec.element_size() == 8        # the 56-byte vector
    s.update([30.0, 31.0], [0.8, 0.9])
    s.update([28.0], [0.7])
    red = s.reduce()
    assert sorted(red) == sorted(['count', 'psnr_iter0', 'ssim_iter0', 'psnr_iter1', 'ssim_iter1', 'psnr_last', 'ssim_last'])
    assert red['count'] == 2 and red['psnr_iter1'] == (31.0 - 1.0) / 2 and red['psnr_last'] == (31.0 + 28.0) / 2


def test_metric_sums_rgb_round_trip_with_a_skipped_iteration():
    from yond_public_amd import distributed as D
    s = D.MetricSums(2, rgb=True)
    assert s.vec.shape == (7 + 3 * 2 + 2,)
    s.update([30.0, 31.0], [0.8, 0.9], [25.0, 26.0], [0.6, 0.7])
    s.update([28.0], [0.7], [24.0, None], [0.5, None])                          # round 2 skipped: its sRGB meter is NOT updated
    s.update([29.0, 29.5], [0.75, 0.76], [23.0, 27.0], [0.55, 0.65])
    red = s.reduce()
    raw = D.MetricSums(2)
    raw.update([30.0, 31.0], [0.8, 0.9]); raw.update([28.0], [0.7]); raw.update([29.0, 29.5], [0.75, 0.76])
    for k, v in raw.reduce().items():
        assert red[k] == v                                                      # the raw meters are untouched
    assert red['psnr_rgb_iter0'] == pytest.approx((25.0 + 24.0 + 23.0) / 3, abs=1e-12)
    assert red['psnr_rgb_iter1'] == pytest.approx((26.0 + 27.0) / 2, abs=1e-12)       # its own count
    assert red['ssim_rgb_iter1'] == pytest.approx((0.7 + 0.65) / 2, abs=1e-12)
    assert red['psnr_rgb_last'] == pytest.approx((26.0 + 24.0 + 27.0) / 3, abs=1e-12)  # the last value that was computed
    assert red['ssim_rgb_last'] == pytest.approx((0.7 + 0.5 + 0.65) / 3, abs=1e-12)
    with pytest.raises(ValueError):
        s.update([30.0], [0.8], [None], [None])


def test_fig_flag_parses_and_defaults_off():
    from yond_public_amd.YOND_SIDD import YONDParser
    a = YONDParser().parse([])
    assert a.fig is False and a.nofig is True
    b = YONDParser().parse(['--fig'])
    assert b.fig is True and b.nofig is True
    c = YONDParser().parse(['--nofig'])
    assert c.fig is False


def test_utils_names():
    from yond_public_amd import utils as U
    from yond_public_amd.utils import sidd_utils, isp_ops
    assert U.process_sidd_image is sidd_utils.process_sidd_image and U.FastISP is isp_ops.FastISP
    import inspect
    sig = inspect.signature(sidd_utils.process_sidd_image)
    assert list(sig.parameters) == ['image', 'bayer_pattern', 'wb', 'cst', 'save_file_rgb']
    assert sig.parameters['save_file_rgb'].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(isp_ops.FastISP)
    assert [(k, p.default) for k, p in sig.parameters.items()][1:] == [('wb', None), ('ccm', None), ('gamma', 2.2)]
